"""float64 restatement of `augment_kernel` (csrc/augment.hip), element by element, with the set of values the kernel may return.

Not to be confused with oracle/augment_ref.py, which restates the REFERENCE's sequential uint8 chain (albumentations over OpenCV) and is what
the kernel is compared with statistically.  This file restates the KERNEL: one packed float32 table [B, NPARAM], one bilinear gather, one
nearest gather, noise, brightness / contrast, HSV.  tests/test_augment_kernel.py anchors it (CPU) to torch indexing, to the oracle's stages and
to the statistics of its noise field; tests/test_gpu_augment.py holds the kernel to it.  Non-square frames test the kernel, not the sampler:
`sample_frame` stays square-only.

Everything is evaluated in float64 from the exact values of the float32 parameters.  A float32 kernel cannot be asked to reproduce a float64
value that sits on a rounding or flooring boundary, so every output element gets ONE value or TWO candidates (a <= b); the report counts the
two-valued ones by reason and the tests cap their share.  u = 2^-24 throughout.

Coordinates.  The kernel forms num = p0 x + p1 y + p2, sw = p6 x + p7 y + p8, sx = num * (1 / sw) in float32 (x, y small integers: exact).  A sum of
three terms carries at most three roundings on the way (two products and two additions, or fewer when the compiler contracts a product into
the addition): |num32 - num| <= 3u A, A = |p0| x + |p1| y + |p2|, and |sw32 - sw| <= 3u D, D = |p6| x + |p7| y + |p8|, to first order.  The reciprocal adds
one rounding: its relative error is 3u D / |sw| + u; the closing product one more: |sx32 - sx| <= 3u A / |sw| + |sx| (2u + 3u D / |sw|).  The band is that,
doubled:  tau_x = 2u (3 A / |sw| + |sx| (2 + 3 D / |sw|)); tau_y, and tau_cx / tau_cy of the second homography (p20 .. p28), are built the same way.
  Refinement (sound, never wider): where every float64 intermediate of that evaluation is itself a float32 number, every float32 operation,
  contracted or not, returns exactly that number, so tau = 0 there.  The Rule X cases (integer shifts, flips, dyadic magnification) live on it:
  their results must be bit-exact, ties included, and the restatement reports nothing two-valued for them.

Image.  v = the float64 bilinear value, zero border.  beta = Lx tau_x + Ly tau_y + 8u 255: Lx, Ly = the largest neighbour differences of the cell
(the slope of the bilinear patch in x and y), 255 for both where sx or sy lies within tau of an integer (the cell itself is then uncertain); the last
term covers the eight float32 roundings of the two lerp levels on values <= 255.  beta = 0 where the coordinates are exact and every intermediate
of the interpolation is a float32 number.  Candidates: rint(clamp(v - beta)) and rint(clamp(v + beta)) (ties to even, as rintf): they differ where a
rounding tie lies within beta of v.  More than two integers in the band (never seen) opens the pixel.

Mask.  The value at (floor(sy + 0.5), floor(sx + 0.5)), 0 outside; where sx + 0.5 or sy + 0.5 lies within tau of an integer the pixel across that
boundary is a candidate too (both: all four).  Equal candidates make the element single-valued after all; more than two distinct values open it.

Crop window.  The kernel tests cx >= p29 - 0.5f, cy >= p30 - 0.5f, cx < p31 - 0.5f, cy < p32 - 0.5f; the four float32 differences are restated bit for bit.
Where a comparison that decides the outcome lies within tau_c of its threshold, 0 and the inside value are both candidates.

Noise.  hash3 and u01 are restated bit for bit (uint32 arithmetic; the one rounding float32 addition of u01 in float32); the Box-Muller term
n = sigma sqrt(-2 ln u1) cos(c u2) in float64 from the float32 u1, u2, sigma and the kernel's float32 constant c = 6.28318530718f.  The band around
the floorf boundaries follows Rule T of tests/sweep_ref.py: 4 x the largest distance from float64 of the same expression evaluated in float32
by numpy on the CPU, per frame, computed here and never taken from the kernel; never below the Rule E bound, k = 8 + 2 operations:
10 u (|px| + |n|).  An element whose px + n lies within the band of an integer is two-valued.

Brightness / contrast.  l alpha + beta 255 in float64 from the float32 alpha, beta; Rule E band k = 5: 5u (|l alpha| + |beta 255|) around the floorf
boundaries; clamped as the kernel clamps.

HSV.  Forward conversion and the three shifts are integer / single float32 operations: exact, one value (the cases keep h + shift away from
integers).  The backward conversion is evaluated in float64 from the integer (h, s, v) and the kernel's float32 constants 6.f / 180.f, 1.f / 255.f;
an element is two-valued where x 255 lies within the Rule E band, k = 8, of a rounding tie.  True ties exist (v = 255, s = 1, h mod 30 = 15).

Chained stages.  A stage that receives a two-valued pixel does not enumerate combinations: the pixel becomes OPEN and is then only asserted to
be a finite integer in [0, 255] (mask: one of {0, 1}).  Open pixels count against the caps.
"""
from dataclasses import dataclass, field

import numpy as np

U = 2.0 ** -24
NPARAM = 36
TWO_PI_F32 = np.float32(6.28318530718)
C_6_180 = np.float32(6.0) / np.float32(180.0)
C_1_255 = np.float32(1.0) / np.float32(255.0)
_M32 = np.uint64(0xFFFFFFFF)


def _is_f32(z):
    with np.errstate(over='ignore', invalid='ignore'):
        return z.astype(np.float32).astype(np.float64) == z


# ------------------------------------------------------------------------------------------------ generator
def hash3(a, b, c):
    """The kernel's counter hash on uint32 values (held in uint64 so that numpy never overflows)."""
    a, b, c = (np.asarray(t, dtype=np.uint64) & _M32 for t in (a, b, c))
    x = ((a * np.uint64(0x9E3779B1)) & _M32) ^ ((((b + np.uint64(0x7F4A7C15)) & _M32) * np.uint64(0x85EBCA77)) & _M32) \
        ^ ((((c + np.uint64(0x165667B1)) & _M32) * np.uint64(0xC2B2AE3D)) & _M32)
    x = x ^ (x >> np.uint64(16)); x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15)); x = (x * np.uint64(0x846CA68B)) & _M32
    return x ^ (x >> np.uint64(16))


def u01(h):
    """((float)(h >> 8) + 0.5f) * 2^-24 in float32: the addition rounds from 2^23 on (so 1.0 can come out, 0.0 cannot)."""
    return ((h >> np.uint64(8)).astype(np.float32) + np.float32(0.5)) * np.float32(1.0 / 16777216.0)


def noise_uniforms(seed, idx):
    """seed: uint32 scalar, idx: flat pixel indices (any shape) -> float32 u1, u2 of shape [3, *idx.shape]."""
    u1 = np.stack([u01(hash3(seed, idx, 2 * c)) for c in range(3)])
    u2 = np.stack([u01(hash3(seed, idx, 2 * c + 1)) for c in range(3)])
    return u1, u2


def noise_field(seed, sigma, idx):
    """float64 Box-Muller term n [3, *idx.shape] from the float32 sigma and the float32 uniforms."""
    u1, u2 = noise_uniforms(seed, idx)
    s = np.float64(np.float32(sigma))
    return s * np.sqrt(-2.0 * np.log(u1.astype(np.float64))) * np.cos(np.float64(TWO_PI_F32) * u2.astype(np.float64))


def noise_field_f32(seed, sigma, idx, px):
    """The yardstick of Rule T: px + sigma * sqrtf(-2.f * logf(u1)) * cosf(c * u2), every operation in float32 (numpy, CPU)."""
    u1, u2 = noise_uniforms(seed, idx)
    return px.astype(np.float32) + np.float32(sigma) * np.sqrt(np.float32(-2.0) * np.log(u1)) * np.cos(TWO_PI_F32 * u2)


# ------------------------------------------------------------------------------------------------ result
@dataclass
class Result:
    img_a: np.ndarray          # float32 [B, 3, H, W]: the lower candidate
    img_b: np.ndarray          # the upper candidate (== img_a where single-valued)
    img_open: np.ndarray       # bool [B, H, W]
    mask_a: np.ndarray         # float32 [B, C, H, W]
    mask_b: np.ndarray
    mask_open: np.ndarray      # bool [B, H, W]
    noise: np.ndarray          # float64 [B, 3, H, W]: the restated field n (0 where sigma == 0)
    noise_yard: np.ndarray     # float64 [B]: the float32 yardstick's largest distance from float64 per frame (0 without noise)
    noise_sum: np.ndarray      # float64 [B, 3, H, W]: px + n before the clamp (0 where sigma == 0)
    report: dict = field(default_factory=dict)

    @property
    def pixels(self):
        return self.img_open.size

    def img_two(self):
        """bool [B, H, W]: some channel two-valued, pixel not open."""
        return (self.img_a != self.img_b).any(1) & ~self.img_open

    def mask_two(self):
        return (self.mask_a != self.mask_b).any(1) & ~self.mask_open

    def shares(self):
        n = float(self.pixels)
        return dict(img_two=self.img_two().sum() / n, img_open=self.img_open.sum() / n, mask_two=self.mask_two().sum() / n,
                    mask_open=self.mask_open.sum() / n, img_two_elements=float((self.img_a != self.img_b).mean()))

    def uncertain_img(self, unit='pixel'):
        """share that counts against an image cap: pixels that are two-valued in any channel or open; unit 'element': elements that are
        two-valued or belong to an open pixel."""
        if unit == 'element':
            return float(((self.img_a != self.img_b) | self.img_open[:, None]).mean())
        return float((self.img_two() | self.img_open).mean())

    def uncertain_mask(self):
        return float((self.mask_two() | self.mask_open).mean())


def compare(res, img_out, mask_out):
    """-> list of failure strings (empty = the outputs are among the candidates).  img_out / mask_out: numpy float32."""
    fails = []
    for name, got, a, b, opn, lo, hi in (('img', img_out, res.img_a, res.img_b, res.img_open, 0.0, 255.0),
                                         ('mask', mask_out, res.mask_a, res.mask_b, res.mask_open, 0.0, 1.0)):
        if got.shape != a.shape:
            fails.append(f'{name}: shape {got.shape}, want {a.shape}')
            continue
        if not np.isfinite(got).all():
            fails.append(f'{name}: {int((~np.isfinite(got)).sum())} elements are not finite (never written, or read out of bounds)')
            continue
        o = np.broadcast_to(opn[:, None], got.shape)
        bad = ~o & (got != a) & (got != b)
        if bad.any():
            i = tuple(int(t[0]) for t in np.nonzero(bad))
            fails.append(f'{name}: {int(bad.sum())} of {bad.size} elements are none of their candidates; first at {i}: got {got[i]!r}, '
                         f'candidates {a[i]!r} | {b[i]!r}')
        wild = o & ((got != np.rint(got)) | (got < lo) | (got > hi))
        if name == 'mask':
            wild = o & (got != 0.0) & (got != 1.0)
        if wild.any():
            fails.append(f'{name}: {int(wild.sum())} open elements outside the output grid')
    return fails


# ------------------------------------------------------------------------------------------------ geometry
def _project(p9, xs, ys):
    """p9 float64 [B, 9] -> (sx, sy, tau_x, tau_y) float64 [B, H, W]."""
    c = [p9[:, k][:, None, None] for k in range(9)]

    def lin(a, b, d):
        t1, t2 = a * xs, b * ys
        s1 = t1 + t2
        s2 = s1 + d
        return s2, np.abs(a) * xs + np.abs(b) * ys + np.abs(d), _is_f32(t1) & _is_f32(t2) & _is_f32(s1) & _is_f32(s2)
    nx, Ax, ex = lin(c[0], c[1], c[2])
    ny, Ay, ey = lin(c[3], c[4], c[5])
    sw, D, ew = lin(c[6], c[7], c[8])
    nz = sw != 0.0
    swd = np.where(nz, sw, 1.0)
    isw = np.where(nz, 1.0 / swd, 0.0)
    sx, sy = np.where(nz, nx / swd, 0.0), np.where(nz, ny / swd, 0.0)
    ei = ew & _is_f32(isw)
    exact_x, exact_y = ex & ei & _is_f32(nx * isw), ey & ei & _is_f32(ny * isw)
    asw = np.abs(swd)
    tx = 2 * U * (3 * Ax / asw + np.abs(sx) * (2 + 3 * D / asw))
    ty = 2 * U * (3 * Ay / asw + np.abs(sy) * (2 + 3 * D / asw))
    return sx, sy, np.where(exact_x, 0.0, tx), np.where(exact_y, 0.0, ty)


def _gather(pl, yy, xx):
    """pl [B, K, H, W], yy / xx int64 [B, H, W] -> float64 [B, K, H, W], 0 outside the frame."""
    B, K, H, W = pl.shape
    ok = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
    v = pl[np.arange(B)[:, None, None], :, np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)]        # [B, H, W, K]
    return np.where(ok[:, None], np.moveaxis(v, -1, 1), 0.0).astype(np.float64)


def _near_int(s, tau):
    return (np.abs(s - np.rint(s)) <= tau) & (tau > 0)


def _geometry(p, img, mask, rep):
    B, _, H, W = img.shape
    xs = np.arange(W, dtype=np.float64)[None, None, :]
    ys = np.arange(H, dtype=np.float64)[None, :, None]
    p64 = p.astype(np.float64)
    sx, sy, tx, ty = _project(p64[:, 0:9], xs, ys)
    cx, cy, tcx, tcy = _project(p64[:, 20:29], xs, ys)
    # ---- crop window: the thresholds are single float32 subtractions
    th = (p[:, 29:33].astype(np.float32) - np.float32(0.5)).astype(np.float64)
    m = [cx - th[:, 0, None, None], cy - th[:, 1, None, None], th[:, 2, None, None] - cx, th[:, 3, None, None] - cy]
    tc = [tcx, tcy, tcx, tcy]
    inside = np.ones(cx.shape, dtype=bool)                       # every comparison holds whatever the rounding
    out = np.zeros(cx.shape, dtype=bool)                         # some comparison fails whatever the rounding
    for mk, tk, strict in zip(m, tc, (False, False, True, True)):
        holds = (mk > 0) if strict else (mk >= 0)
        inside &= np.where(tk > 0, mk > tk, holds)
        out |= np.where(tk > 0, mk < -tk, ~holds)
    crop_unc = ~inside & ~out
    # ---- image
    x0f, y0f = np.floor(sx), np.floor(sy)
    big = 2.0 ** 40
    x0, y0 = np.clip(x0f, -big, big).astype(np.int64), np.clip(y0f, -big, big).astype(np.int64)
    ax, ay = (sx - x0f)[:, None], (sy - y0f)[:, None]
    v00, v01, v10, v11 = _gather(img, y0, x0), _gather(img, y0, x0 + 1), _gather(img, y0 + 1, x0), _gather(img, y0 + 1, x0 + 1)
    wx, wy = 1.0 - ax, 1.0 - ay
    t1, t2, b1, b2 = v00 * wx, v01 * ax, v10 * wx, v11 * ax
    top, bot = t1 + t2, b1 + b2
    u1, u2 = top * wy, bot * ay
    v = u1 + u2
    exact = ((tx == 0) & (ty == 0))[:, None]
    for z in (wx, wy, t1, t2, b1, b2, top, bot, u1, u2, v):
        exact = exact & _is_f32(z)
    cell_unc = (_near_int(sx, tx) | _near_int(sy, ty))[:, None]
    Lx = np.where(cell_unc, 255.0, np.maximum(np.abs(v01 - v00), np.abs(v11 - v10)))
    Ly = np.where(cell_unc, 255.0, np.maximum(np.abs(v10 - v00), np.abs(v11 - v01)))
    beta = np.where(exact, 0.0, Lx * tx[:, None] + Ly * ty[:, None] + 8 * U * 255.0)
    lo, hi = np.rint(np.clip(v - beta, 0.0, 255.0)), np.rint(np.clip(v + beta, 0.0, 255.0))
    rep['img_tie'] = rep.get('img_tie', 0) + int(((lo != hi).any(1) & ~out).sum())
    rep['img_cell'] = rep.get('img_cell', 0) + int(((lo != hi).any(1) & ~out & cell_unc[:, 0]).sum())
    img_open = (hi - lo > 1).any(1) & ~out
    lo, hi = np.where(out[:, None], 0.0, lo), np.where(out[:, None], 0.0, hi)
    cu = crop_unc[:, None]
    img_open |= (crop_unc[:, None] & (lo != hi) & (lo != 0)).any(1)
    rep['img_crop'] = rep.get('img_crop', 0) + int((cu & (hi != 0)).any(1).sum())
    lo = np.where(cu, 0.0, lo)
    # ---- mask
    hx, hy = sx + 0.5, sy + 0.5
    mxf, myf = np.floor(hx), np.floor(hy)
    mx, my = np.clip(mxf, -big, big).astype(np.int64), np.clip(myf, -big, big).astype(np.int64)
    # the pixel across the boundary: below when the sum sits just above an integer, above when just below
    altx = np.where(_near_int(hx, tx), np.where(hx - mxf <= 0.5, mx - 1, mx + 1), mx)
    alty = np.where(_near_int(hy, ty), np.where(hy - myf <= 0.5, my - 1, my + 1), my)
    g = np.stack([_gather(mask, my, mx), _gather(mask, my, altx), _gather(mask, alty, mx), _gather(mask, alty, altx)])
    mlo, mhi = g.min(0), g.max(0)
    mask_open = ((g != mlo) & (g != mhi)).any(0).any(1)
    mask_open &= ~out
    rep['mask_nearest'] = rep.get('mask_nearest', 0) + int(((mlo != mhi).any(1) & ~out).sum())
    mlo, mhi = np.where(out[:, None], 0.0, mlo), np.where(out[:, None], 0.0, mhi)
    mask_open |= (cu & (mlo != mhi) & (mlo != 0)).any(1)
    rep['mask_crop'] = rep.get('mask_crop', 0) + int((cu & (mhi != 0)).any(1).sum())
    mlo = np.where(cu, np.minimum(mlo, 0.0), mlo)
    mhi = np.where(cu, np.maximum(mhi, 0.0), mhi)
    return lo, hi, img_open, mlo, mhi, mask_open


def _enter_stage(a, b, opn, active):
    """A photometric stage on the frames `active`: two-valued pixels become open; the stage goes on from the lower candidate."""
    two = (a != b).any(1) & active[:, None, None]
    opn |= two
    return np.where(two[:, None], a, b)


# ------------------------------------------------------------------------------------------------ photometric stages
def _noise(p, a, b, opn, n0, rep):
    B, _, H, W = a.shape
    sigma = p[:, 11].astype(np.float32)
    active = sigma > 0
    field_, sums, yard = np.zeros(a.shape), np.zeros(a.shape), np.zeros(B)
    if not active.any():
        return a, b, field_, yard, sums
    b = _enter_stage(a, b, opn, active)
    seeds = np.ascontiguousarray(p[:, 12].astype(np.float32, copy=False)).view(np.uint32)
    a, b = a.copy(), b.copy()
    for n in np.nonzero(active)[0]:
        idx = ((np.uint64(n0 + n) * np.uint64(H * W) + np.arange(H * W, dtype=np.uint64)) & _M32).reshape(H, W)     # (unsigned)i
        nf = noise_field(seeds[n], sigma[n], idx)
        s = a[n] + nf
        yard[n] = np.abs(noise_field_f32(seeds[n], sigma[n], idx, a[n]).astype(np.float64) - s).max()
        band = np.maximum(4.0 * yard[n], 10 * U * (np.abs(a[n]) + np.abs(nf)))
        a[n], b[n] = np.floor(np.clip(s - band, 0.0, 255.0)), np.floor(np.clip(s + band, 0.0, 255.0))
        field_[n], sums[n] = nf, s
        rep['noise'] = rep.get('noise', 0) + int((a[n] != b[n]).sum())
    return a, b, field_, yard, sums


def _brightness_contrast(p, a, b, opn, rep):
    alpha, beta = p[:, 9].astype(np.float32), p[:, 10].astype(np.float32)
    active = (alpha != 1) | (beta != 0)
    if not active.any():
        return a, b
    b = _enter_stage(a, b, opn, active)
    al, be = alpha.astype(np.float64)[:, None, None, None], beta.astype(np.float64)[:, None, None, None] * 255.0
    val = a * al + be
    band = 5 * U * (np.abs(a * al) + np.abs(be))
    act = active[:, None, None, None]
    lo, hi = np.floor(np.clip(val - band, 0.0, 255.0)), np.floor(np.clip(val + band, 0.0, 255.0))
    rep['bc'] = rep.get('bc', 0) + int(((lo != hi) & act).sum())
    return np.where(act, lo, a), np.where(act, hi, b)


def rgb2hsv_int(r, g, b):
    """OpenCV's 8-bit forward conversion, H in [0, 180): integer arithmetic with the 12-bit reciprocal tables."""
    v = np.maximum(r, np.maximum(g, b))
    diff = v - np.minimum(r, np.minimum(g, b))
    sdiv = np.where(v > 0, np.rint(255.0 * 4096.0 / np.maximum(v, 1)), 0).astype(np.int64)
    hdiv = np.where(diff > 0, np.rint(180.0 * 4096.0 / (6.0 * np.maximum(diff, 1))), 0).astype(np.int64)
    s = (diff * sdiv + 2048) >> 12
    hh = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    hh = (hh * hdiv + 2048) >> 12
    return np.where(hh < 0, hh + 180, hh), s, v


def _hsv(p, a, b, opn, rep):
    with np.errstate(invalid='ignore'):
        active = (np.nan_to_num(p[:, 16].astype(np.float64)).astype(np.int64) & 1) == 1
    if not active.any():
        return a, b
    b = _enter_stage(a, b, opn, active)
    fr = np.nonzero(active)[0]
    px = a[fr].astype(np.int64)
    h, s, v = rgb2hsv_int(px[:, 0], px[:, 1], px[:, 2])
    hs, ss, vs = (p[fr, k].astype(np.float32)[:, None, None] for k in (13, 14, 15))
    # the three shifts: one float32 addition each, fmodf (exact), truncation
    t = np.fmod(h.astype(np.float32) + hs, np.float32(180.0))
    t = np.where(t < 0, t + np.float32(180.0), t)
    h = np.where(hs != 0, t.astype(np.int64), h)
    s = np.where(ss != 0, np.clip(s.astype(np.float32) + ss, np.float32(0), np.float32(255)).astype(np.int64), s)
    v = np.where(vs != 0, np.clip(v.astype(np.float32) + vs, np.float32(0), np.float32(255)).astype(np.int64), v)
    # backward, float64 from the float32 constants
    fs, fv = s * np.float64(C_1_255), v * np.float64(C_1_255)
    hf = h * np.float64(C_6_180)
    hf = np.where(hf >= 6.0, hf - 6.0, hf)
    sector = np.floor(hf)
    fh = hf - sector
    bad = (sector < 0) | (sector >= 6)
    sector, fh = np.where(bad, 0, sector).astype(np.int64), np.where(bad, 0.0, fh)
    mh = hf + sector                                             # |hh| + |sector|: the magnitude of the subtraction
    tab = np.stack([fv, fv * (1 - fs), fv * (1 - fs * fh), fv * (1 - fs * (1 - fh))])
    mag = np.stack([fv, fv * (1 + fs), fv * (1 + fs * mh), fv * (1 + fs * (1 + mh))])
    sd = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])      # (b, g, r) -> index into tab
    pick = sd[sector]                                            # [n, H, W, 3]
    grey = s == 0
    lo, hi = np.empty(px.shape), np.empty(px.shape)
    for ch, k in ((0, 2), (1, 1), (2, 0)):                       # output channel 0 = "R" = column 2 of the sector table
        sel = pick[..., k][None]
        x = np.where(grey, fv, np.take_along_axis(tab, sel, 0)[0]) * 255.0
        band = 8 * U * np.where(grey, fv, np.take_along_axis(mag, sel, 0)[0]) * 255.0
        lo[:, ch], hi[:, ch] = np.clip(np.rint(x - band), 0, 255), np.clip(np.rint(x + band), 0, 255)
    rep['hsv'] = rep.get('hsv', 0) + int((lo != hi).sum())
    a, b = a.copy(), b.copy()
    a[fr], b[fr] = lo, hi
    return a, b


# ------------------------------------------------------------------------------------------------ entry
def augment_ref(params, img, mask):
    """params float32 [B, NPARAM], img [B, 3, H, W], mask [B, C, H, W] (numpy or torch, float32) -> Result."""
    p = np.ascontiguousarray(np.asarray(params, dtype=np.float32))
    img, mask = np.asarray(img, dtype=np.float32), np.asarray(mask, dtype=np.float32)
    B, _, H, W = img.shape
    chunk = max(1, (1 << 19) // (H * W))                         # frames per pass: bounds the float64 temporaries
    assert p.shape == (B, NPARAM) and mask.shape[0] == B and mask.shape[2:] == (H, W)
    rep = {}
    parts = []
    for n0 in range(0, B, chunk):
        sl = slice(n0, min(B, n0 + chunk))
        a, b, opn, ma, mb, mopn = _geometry(p[sl], img[sl], mask[sl], rep)
        a, b, nf, yard, sums = _noise(p[sl], a, b, opn, n0, rep)
        a, b = _brightness_contrast(p[sl], a, b, opn, rep)
        a, b = _hsv(p[sl], a, b, opn, rep)
        parts.append((a.astype(np.float32), b.astype(np.float32), opn, ma.astype(np.float32), mb.astype(np.float32), mopn, nf, yard, sums))
    cat = [np.concatenate([q[k] for q in parts]) for k in range(9)]
    res = Result(cat[0], cat[1], cat[2], cat[3], cat[4], cat[5], cat[6], cat[7], cat[8], rep)
    rep.update({k: int(v) for k, v in dict(img_two_pixels=res.img_two().sum(), img_open_pixels=res.img_open.sum(),
                                           mask_two_pixels=res.mask_two().sum(), mask_open_pixels=res.mask_open.sum(), pixels=res.pixels).items()})
    return res
