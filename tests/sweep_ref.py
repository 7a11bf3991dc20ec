"""float64 references of the NHWC sweep kernels, the comparison rules of their single-op tests, and the guarded buffers.

Every reference is a plain torch restatement of one launcher of csrc/kernels.h on NHWC tensors, evaluated in float64 on
inputs that were first rounded to the tested storage dtype T.  tests/test_sweeps.py checks the references against
torch.nn.functional / autograd (CPU, NCHW, float64); tests/test_gpu_sweeps.py checks the kernels against the references.

Comparison rules (u_T = unit roundoff of T: 2^-24 f32, 2^-8 bf16, 2^-11 f16; eps32 = 2^-24):
  X  exact.  Inputs are dyadic (small integers times a power of two), per-channel factors powers of two or small integers:
     every f32 intermediate and partial sum is representable whatever the order, so the kernel must return the float64
     reference rounded once to T, bit for bit (integer views are compared).
  E  element-wise.  |got - ref| <= u_T |ref| + k eps32 mag, mag = the expression with every term replaced by its absolute
     value, k = f32 operations of the kernel's expression + 2.
  R  reductions over n terms.  |got - ref| <= n eps32 sum|terms| (+ u_T |ref| when stored as T).  n counts the terms that are
     added, an accumulated destination included; a closing division replaces the missing n-th addition.  Where the kernel forms a
     term by rounded float operations of its own, the random cases are kept to outputs with at least 8 terms (the Rule X twins
     carry the short sums), or the reference forms the term from the very float the kernel uses (bilinear adjoint weights).
  (stored as T: u_T |ref|, or half the spacing of T's subnormal numbers where |ref| lies below T's smallest normal number.)
  T  transcendentals (sigmoid, exp, square root).  The yardstick is the same expression evaluated by torch on the CPU in
     float32 (stored as T); the kernel's largest distance from float64 may be 4 x the yardstick's largest distance, and
     never has to beat the Rule E bound.
"""
import math

import torch
import torch.nn.functional as F

EPS32 = 2.0 ** -24
U = {torch.float32: 2.0 ** -24, torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11}
VEC = {torch.float32: 4, torch.bfloat16: 8, torch.float16: 8}
INT_VIEW = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float16: torch.int16}
DTYPE_NAMES = {torch.float32: 'f32', torch.bfloat16: 'bf16', torch.float16: 'f16'}


# ------------------------------------------------------------------------------------------------ inputs
def gen(seed):
    return torch.Generator().manual_seed(seed)


def normal(shape, dtype, g, scale=1.0):
    """Random normal values rounded to T (the kernel and the reference then start from the same numbers)."""
    return (torch.randn(shape, generator=g, dtype=torch.float64) * scale).to(torch.float32).to(dtype)


def dyadic(shape, dtype, g, lo=-8, hi=8, step=0.25):
    """Rule X values: integers in [lo, hi] times `step` (a power of two): exact in every T (at most 5 significant bits)."""
    return (torch.randint(lo, hi + 1, shape, generator=g).to(torch.float64) * step).to(dtype)


def pow2(shape, g, lo=-2, hi=2, signed=True):
    """Rule X per-channel factors: +-2^e, lo <= e <= hi (float32)."""
    v = torch.pow(2.0, torch.randint(lo, hi + 1, shape, generator=g).to(torch.float64))
    if signed:
        v = v * (torch.randint(0, 2, shape, generator=g).to(torch.float64) * 2 - 1)
    return v.to(torch.float32)


def ints(shape, g, lo=-4, hi=4):
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.float32)


REF_DTYPE = [torch.float64]   # float32 while test_sweeps.py proves that the Rule X input sets are exact (as_float32)


class as_float32:
    """Evaluate the references in float32 instead of float64 (Rule X sets must give the same numbers both ways)."""

    def __enter__(self):
        REF_DTYPE[0] = torch.float32

    def __exit__(self, *a):
        REF_DTYPE[0] = torch.float64


def d(t):
    return None if t is None else t.detach().cpu().to(REF_DTYPE[0])


# ------------------------------------------------------------------------------------------------ comparison helpers
def round_once(ref64, dtype):
    """float64 -> T with ONE rounding.  torch converts double -> bf16 / f16 through float, so the value has to be a float32
    already (Rule X guarantees it; asserted)."""
    f = ref64.to(torch.float32)
    if dtype != torch.float32:
        assert torch.equal(f.to(torch.float64), ref64.to(torch.float64)), 'reference is not exact in float32: not a Rule X case'
    return f.to(dtype)


def is_f32_exact(ref64):
    return torch.equal(ref64.to(torch.float32).to(torch.float64), ref64)


def bits_of(t):
    return t.contiguous().view(INT_VIEW[t.dtype])


def assert_exact(got, ref64, what=''):
    """Rule X: got (a tensor of T) equals the float64 reference rounded once to T, bit for bit."""
    got = got.detach().cpu()
    if not got.dtype.is_floating_point:      # mask bits, pool indices
        want = ref64.reshape(got.shape).to(got.dtype)
        assert torch.equal(got, want), f'{what}: {int((got != want).sum())} of {got.numel()} bytes differ'
        return
    want = round_once(ref64.reshape(got.shape), got.dtype)
    gb, wb = bits_of(got), bits_of(want)
    if not torch.equal(gb, wb):
        bad = (gb != wb).reshape(-1).nonzero().reshape(-1)
        i = int(bad[0])
        raise AssertionError(f'{what}: {bad.numel()} of {gb.numel()} elements differ bit-wise; first at flat index {i}: '
                             f'got {got.reshape(-1)[i].item()!r}, want {want.reshape(-1)[i].item()!r}')


# half the spacing of T's subnormal numbers: below the smallest normal number the spacing no longer shrinks with the value, so the rounding
# to T is bounded by this instead of u_T |ref| (f16: results below 2^-14 = 6.1e-5, e.g. a resampled ReLU output next to zero)
SUBNORMAL_HALF = {torch.float32: 2.0 ** -150, torch.bfloat16: 2.0 ** -134, torch.float16: 2.0 ** -25}


def storage_error(ref64, dtype):
    return (U[dtype] * ref64.abs()).clamp_min(SUBNORMAL_HALF[dtype])


def bound_e(ref64, mag64, k, dtype, stored=True):
    return (storage_error(ref64, dtype) if stored else 0.0) + k * EPS32 * mag64


def bound_r(ref64, sumabs64, n, dtype=None):
    b = n * EPS32 * sumabs64
    return b + storage_error(ref64, dtype) if dtype is not None else b


def assert_within(got, ref64, bound64, what=''):
    g64 = d(got).reshape(ref64.shape)
    err = (g64 - ref64).abs()
    ok = err <= bound64          # a NaN (an element nobody wrote, or an out-of-bounds read) fails here
    if not bool(ok.all()):
        bad = (~ok).reshape(-1).nonzero().reshape(-1)
        i = int(bad[0])
        bnd = bound64.reshape(-1)[i].item() if torch.is_tensor(bound64) and bound64.numel() > 1 else float(bound64)
        raise AssertionError(f'{what}: {bad.numel()} of {ok.numel()} elements out of bound; first at flat index {i}: got '
                             f'{g64.reshape(-1)[i].item()!r}, ref {ref64.reshape(-1)[i].item()!r}, bound {bnd!r}')


RATIOS = []   # (op, dtype name, ratio): printed by the GPU module when it finishes


def assert_transcendental(got, ref64, yard, bound_e64, what, dtype):
    """Rule T.  yard: the float32 CPU evaluation (already stored as T where the kernel stores T)."""
    g64 = d(got).reshape(ref64.shape)
    ydist = float((d(yard).reshape(ref64.shape) - ref64).abs().max())
    kdist = float((g64 - ref64).abs().max())
    ratio = kdist / ydist if ydist > 0 else (0.0 if kdist == 0 else math.inf)
    RATIOS.append((what, DTYPE_NAMES[dtype], ratio))
    print(f'transcendental ratio {what} {DTYPE_NAMES[dtype]}: kernel {kdist:.3e} / float32 yardstick {ydist:.3e} = {ratio:.3f}')
    assert_within(got, ref64, torch.maximum(torch.full_like(ref64, 4.0 * ydist), bound_e64), what)


# ------------------------------------------------------------------------------------------------ guarded buffers
MARGIN = 4096
FILL = 0xFF      # 0xFFFF.. is a NaN in f32, bf16, f16 and f64; as bytes it is the fixed pattern of the byte margins


class Guard:
    """Device tensors as 16-byte-aligned interior views of larger allocations with 4 KiB margins either side.  The margins (and,
    for `empty`, the interior) are filled with 0xFF bytes = NaN; `check()` asserts that no margin byte changed."""

    def __init__(self, device):
        self.device = device
        self.bufs = []

    def _alloc(self, shape, dtype):
        n = 1
        for s in shape:
            n *= int(s)
        nbytes = n * torch.empty((), dtype=dtype).element_size()
        padded = (nbytes + 15) // 16 * 16
        buf = torch.full((MARGIN + padded + MARGIN,), FILL, dtype=torch.uint8, device=self.device)
        assert buf.data_ptr() % 16 == 0
        view = buf[MARGIN:MARGIN + nbytes].view(dtype).view(*shape)
        assert view.data_ptr() % 16 == 0
        self.bufs.append((buf, nbytes))
        return view

    def put(self, t):
        """A guarded device copy of the CPU tensor t (None stays None)."""
        if t is None:
            return None
        v = self._alloc(tuple(t.shape), t.dtype)
        v.copy_(t)
        return v

    def empty(self, shape, dtype):
        """A guarded output: every element starts as NaN (0xFF for bytes), so one that nobody wrote shows."""
        return self._alloc(tuple(shape), dtype)

    def zeros(self, shape, dtype):
        v = self._alloc(tuple(shape), dtype)
        v.zero_()
        return v

    def check(self):
        for buf, nbytes in self.bufs:
            assert bool((buf[:MARGIN] == FILL).all()), 'a kernel wrote in front of a buffer'
            assert bool((buf[MARGIN + nbytes:] == FILL).all()), 'a kernel wrote behind a buffer'


# ------------------------------------------------------------------------------------------------ BatchNorm finalize
def bn_stats_from_sums(s1, s2, count, gamma, beta, rm, rv, momentum, eps):
    """mean / var from (sum, sum of squares) as bn_finalize_train does; everything float64.  Returns a dict."""
    mean = s1 / count
    var = (s2 / count - mean * mean).clamp_min(0.0)
    return _bn_outputs(mean, var, var * count / (count - 1.0) if count > 1 else var, gamma, beta, rm, rv, momentum, eps)


def _bn_outputs(mean, var, unbiased, gamma, beta, rm, rv, momentum, eps):
    rstd = 1.0 / torch.sqrt(var + eps)
    scale = gamma * rstd
    return dict(mean=mean, rstd=rstd, scale=scale, shift=beta - mean * scale, running_mean=(1 - momentum) * rm + momentum * mean,
                running_var=(1 - momentum) * rv + momentum * unbiased)


def bn_finalize_train(slab, count, gamma, beta, rm, rv, momentum, eps):
    s = d(slab)
    return bn_stats_from_sums(s[..., 0].sum(0), s[..., 1].sum(0), float(count), d(gamma), d(beta), d(rm), d(rv), momentum, eps)


def bn_finalize_small(y, gamma, beta, rm, rv, momentum, eps):
    y = d(y)
    n = y.shape[0]
    mean = y.mean(0)
    ssd = ((y - mean) ** 2).sum(0)
    return _bn_outputs(mean, ssd / n, ssd / (n - 1) if n > 1 else ssd / n, d(gamma), d(beta), d(rm), d(rv), momentum, eps)


def bn_finalize_eval(gamma, beta, rm, rv, eps):
    sd = torch.sqrt(d(rv) + eps)
    scale = d(gamma) / sd
    return dict(scale=scale, shift=d(beta) - d(rm) * scale, mean=d(rm), rstd=1.0 / sd)


# ------------------------------------------------------------------------------------------------ BatchNorm apply
BN_ACT_K = 4 + 2      # fma (scale, shift), fma (rscale, rshift), + res, + post


def bn_act(y, scale=None, shift=None, res=None, rscale=None, rshift=None, post=None, relu=False):
    """-> (out, mag, maskbits): float64 [npix, C]; maskbits = one byte per 16-byte vector is made by `pack_mask`."""
    x = d(y)
    mag = x.abs()
    if scale is not None:
        x, mag = x * d(scale) + d(shift), mag * d(scale).abs() + d(shift).abs()
    if res is not None:
        r = d(res)
        rm_ = r.abs()
        if rscale is not None:
            r, rm_ = r * d(rscale) + d(rshift), rm_ * d(rscale).abs() + d(rshift).abs()
        x, mag = x + r, mag + rm_
    if relu:
        x = torch.where(x < 0, torch.zeros_like(x), x)
    if post is not None:
        x, mag = x + d(post), mag + d(post).abs()
    return x, mag


def pack_mask(pos, vec):
    """bool [npix, C] -> uint8 [npix, C / vec]: bit i = element i of the vector."""
    npix, Cn = pos.shape
    w = (2 ** torch.arange(vec, dtype=torch.int64)).view(1, 1, vec)
    return (pos.view(npix, Cn // vec, vec).to(torch.int64) * w).sum(-1).to(torch.uint8)


# ------------------------------------------------------------------------------------------------ BatchNorm backward
def bn_bwd_mask(g, y, mask, scale=None, shift=None, out=None, maskpos=None):
    """dz = g * mask (float64): mask 0 none, 1 fma(y, scale, shift) > 0 (evaluated as the kernel does, one float32 fma),
    2 out > 0 or the saved mask bits (maskpos: bool)."""
    g = d(g)
    if mask == 1:
        z = (d(y) * d(scale) + d(shift)).to(torch.float32)     # a float32 fma = the float64 value rounded once
        return torch.where(z > 0, g, torch.zeros_like(g))
    if mask == 2:
        pos = maskpos if maskpos is not None else d(out) > 0
        return torch.where(pos, g, torch.zeros_like(g))
    return g




def bn_bwd_row_of_pixel(npix, rows, tpv):
    """slab row that bn_bwd_reduce adds pixel p into: workgroup (p / tpv) mod rows."""
    return (torch.arange(npix) // tpv) % rows


def bn_bwd_reduce(dz, y, mean, rstd, rows, tpv):
    """-> slab [rows, C, 2], sumabs [rows, C, 2], n [rows] (terms per row)."""
    y = d(y)
    npix, Cn = y.shape
    t2 = dz * (y - d(mean)) * d(rstd)
    a2 = dz.abs() * (y.abs() + d(mean).abs()) * d(rstd).abs()
    row = bn_bwd_row_of_pixel(npix, rows, tpv)
    slab = torch.zeros(rows, Cn, 2, dtype=REF_DTYPE[0])
    sa = torch.zeros(rows, Cn, 2, dtype=REF_DTYPE[0])
    slab[..., 0].index_add_(0, row, dz)
    slab[..., 1].index_add_(0, row, t2)
    sa[..., 0].index_add_(0, row, dz.abs())
    sa[..., 1].index_add_(0, row, a2)
    n = torch.zeros(rows, dtype=REF_DTYPE[0]).index_add_(0, row, torch.ones(npix, dtype=REF_DTYPE[0]))
    return slab, sa, n


BN_APPLY_K = 7 + 2    # A = gamma rstd; (y - mean), * rstd, * c2; g - c1, - ..., A * ...


def bn_bwd_apply(dz, y, mean, rstd, gamma, coef):
    y, mu, rs, A = d(y), d(mean), d(rstd), d(gamma) * d(rstd)
    c = d(coef).view(-1, 2)
    c1, c2 = c[:, 0], c[:, 1]
    ref = A * (dz - c1 - (y - mu) * rs * c2)
    mag = A.abs() * (dz.abs() + c1.abs() + (y.abs() + mu.abs()) * rs.abs() * c2.abs())
    return ref, mag


def bn_backward_autograd(x, g, gamma, beta, eps, relu):
    """d/dx, dgamma, dbeta of sum(g * act(batch_norm(x))) by autograd, float64, x [npix, C]."""
    x = d(x).clone().requires_grad_(True)
    ga = d(gamma).clone().requires_grad_(True)
    be = d(beta).clone().requires_grad_(True)
    z = F.batch_norm(x.t().unsqueeze(0), None, None, ga, be, True, 0.0, eps)[0].t()
    if relu:
        z = F.relu(z)
    (z * d(g)).sum().backward()
    return x.grad, ga.grad, be.grad


# ------------------------------------------------------------------------------------------------ plumbing
def pool2x2(src):
    s = d(src)
    return s[:, 0::2, 0::2] + s[:, 0::2, 1::2] + s[:, 1::2, 0::2] + s[:, 1::2, 1::2]


def up2(x):
    return d(x).repeat_interleave(2, 1).repeat_interleave(2, 2)


def to_nchw(x):
    return x.permute(0, 3, 1, 2)


def to_nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def tensor_stats_row(npix, rows, tpv):
    return (torch.arange(npix) // tpv) % rows


# ------------------------------------------------------------------------------------------------ maxpool 3x3 s2 p1
def maxpool_fwd(x):
    """-> (out float64 [N, H/2, W/2, C], idx uint8: window position 3 r + s of the FIRST maximum in scan order)."""
    x = d(x)
    N, H, W, Cn = x.shape
    OH, OW = H // 2, W // 2
    best = torch.full((N, OH, OW, Cn), -math.inf, dtype=REF_DTYPE[0])
    idx = torch.full((N, OH, OW, Cn), 255, dtype=torch.uint8)
    xp = F.pad(x, (0, 0, 1, 1, 1, 1), value=-math.inf)      # (the border never wins: a maximum has to be greater than -inf)
    for r in range(3):
        for s in range(3):
            win = xp[:, r:r + 2 * OH:2, s:s + 2 * OW:2]
            take = win > best
            best = torch.where(take, win, best)
            idx = torch.where(take, torch.full_like(idx, 3 * r + s), idx)
    return best, idx


def maxpool_bwd(idx, gout, H, W):
    """gin[n, 2 oy - 1 + r, 2 ox - 1 + s, c] += gout[n, oy, ox, c] where idx == 3 r + s."""
    g = d(gout)
    N, OH, OW, Cn = g.shape
    gin = torch.zeros(N, H + 2, W + 2, Cn, dtype=REF_DTYPE[0])
    for r in range(3):
        for s in range(3):
            gin[:, r:r + 2 * OH:2, s:s + 2 * OW:2] += torch.where(idx == 3 * r + s, g, torch.zeros_like(g))
    return gin[:, 1:H + 1, 1:W + 1].contiguous()


# ------------------------------------------------------------------------------------------------ bilinear, align_corners=True
LERP_FUSED = [False]


def lerp_table(n_in, n_out):
    """torch's align_corners=True source index in float32: scale = (in - 1) / (out - 1) (0 when out == 1), x = scale * o, i0 = int(x),
    w1 = x - i0, w0 = 1 - w1.  Two evaluations of w1 exist: torch's CPU kernels round the product x before they subtract i0
    (LERP_FUSED off); a compiler that contracts the product into the subtraction computes fma(scale, o, -i0), one rounding
    (LERP_FUSED on).  A kernel has to agree with ONE of them everywhere (either_weights).  -> i0, i1, w0, w1 (float32 values)."""
    scale = torch.tensor((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0, dtype=torch.float64).to(torch.float32)
    o = torch.arange(n_out, dtype=torch.float32)
    x = scale * o
    i0 = x.to(torch.int64).clamp_max(n_in - 1)
    i1 = i0 + (i0 < n_in - 1).to(torch.int64)
    if LERP_FUSED[0]:      # the product of a 24-bit and a small integer is exact in float64
        w1 = (scale.to(torch.float64) * o.to(torch.float64) - i0.to(torch.float64)).to(torch.float32)
    else:
        w1 = x - i0.to(torch.float32)
    w0 = 1.0 - w1
    return i0, i1, w0.to(REF_DTYPE[0]), w1.to(REF_DTYPE[0])


def either_weights(check):
    """Run check() with the rounded-product weights, then with the fused ones; every element has to pass under one of the two."""
    try:
        check()
        return
    except AssertionError as first:
        LERP_FUSED[0] = True
        try:
            check()
        except AssertionError as second:
            raise AssertionError(f'rounded-product weights: {first}; fused weights: {second}')
        finally:
            LERP_FUSED[0] = False


BILINEAR_K = 9 + 2    # four products and two sums inside, two products and a sum outside


def bilinear_resize(x, OH, OW):
    """-> (out, mag) float64 [N, OH, OW, C] with the float32 weights of lerp_table."""
    x = d(x)
    y0, y1, wy0, wy1 = lerp_table(x.shape[1], OH)
    x0, x1, wx0, wx1 = lerp_table(x.shape[2], OW)
    wy0, wy1 = wy0.view(1, OH, 1, 1), wy1.view(1, OH, 1, 1)
    wx0, wx1 = wx0.view(1, 1, OW, 1), wx1.view(1, 1, OW, 1)

    def ev(t):
        top = wx0 * t[:, y0][:, :, x0] + wx1 * t[:, y0][:, :, x1]
        bot = wx0 * t[:, y1][:, :, x0] + wx1 * t[:, y1][:, :, x1]
        return wy0 * top + wy1 * bot
    return ev(x), ev(x.abs())


def bilinear_matrix(n_in, n_out):
    """[n_out, n_in] matrix of the one-axis resample: the float32 weight sums the adjoint kernels form
    ((i0 == i ? w0 : 0) + (i1 == i ? w1 : 0))."""
    i0, i1, w0, w1 = lerp_table(n_in, n_out)
    m = torch.zeros(n_out, n_in, dtype=torch.float32)
    m[torch.arange(n_out), i0] += w0.to(torch.float32)
    m[torch.arange(n_out), i1] += w1.to(torch.float32)
    return m.to(REF_DTYPE[0])


def bilinear_adjoint(gout, IH, IW, float_products=False):
    """-> (gin, sumabs, nterms [IH, IW]): the transpose of bilinear_resize.  float_products: the weight of a term is the float32
    product wy * wx the kernels form, so that a term carries no rounding of its own and only its addition (one fma) rounds."""
    g = d(gout)
    my, mx = bilinear_matrix(IH, g.shape[1]), bilinear_matrix(IW, g.shape[2])
    nt = (my != 0).sum(0).view(-1, 1) * (mx != 0).sum(0).view(1, -1)
    if float_products:
        w = (my.view(-1, IH, 1, 1) * mx.view(1, 1, -1, IW)).to(torch.float32).to(REF_DTYPE[0])      # [OH, IH, OW, IW]
        f = lambda t: torch.einsum('oipj,nopc->nijc', w, t)
    else:
        f = lambda t: torch.einsum('pj,nipc->nijc', mx, torch.einsum('oi,nopc->nipc', my, t))
    return f(g), f(g.abs()), nt.to(REF_DTYPE[0])


# ------------------------------------------------------------------------------------------------ adaptive average pooling
def bin_range(i, k, H):
    return (i * H) // k, ((i + 1) * H + k - 1) // k


def bin_mean(x, k):
    """-> (out, sumabs, count) [N, k, k, C]"""
    x = d(x)
    N, H, W, Cn = x.shape
    out = torch.zeros(N, k, k, Cn, dtype=REF_DTYPE[0])
    sa = torch.zeros_like(out)
    cnt = torch.zeros(k, k, dtype=REF_DTYPE[0])
    for i in range(k):
        y0, y1 = bin_range(i, k, H)
        for j in range(k):
            x0, x1 = bin_range(j, k, W)
            n = (y1 - y0) * (x1 - x0)
            out[:, i, j] = x[:, y0:y1, x0:x1].sum((1, 2)) / n
            sa[:, i, j] = x[:, y0:y1, x0:x1].abs().sum((1, 2)) / n
            cnt[i, j] = n
    return out, sa, cnt


def bin_mean_bwd(gout, H, W):
    """-> (gin, sumabs, nterms) [N, H, W, C]: every bin that holds the pixel adds gout[bin] * float32(1 / area)."""
    g = d(gout)
    N, k, _, Cn = g.shape
    gin = torch.zeros(N, H, W, Cn, dtype=REF_DTYPE[0])
    sa = torch.zeros_like(gin)
    nt = torch.zeros(H, W, dtype=REF_DTYPE[0])
    for i in range(k):
        y0, y1 = bin_range(i, k, H)
        for j in range(k):
            x0, x1 = bin_range(j, k, W)
            inv = float(torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float((y1 - y0) * (x1 - x0)), dtype=torch.float32))
            gin[:, y0:y1, x0:x1] += g[:, i, j].view(N, 1, 1, Cn) * inv
            sa[:, y0:y1, x0:x1] += g[:, i, j].abs().view(N, 1, 1, Cn) * inv
            nt[y0:y1, x0:x1] += 1
    return gin, sa, nt


# ------------------------------------------------------------------------------------------------ gates
def sigmoid_as_kernel(z):
    """sigmoid_acc of csrc/sigmoid.h in the dtype of z (float64 reference, float32 yardstick)."""
    e = torch.exp(-z.abs())
    return torch.where(z >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


SE_GATE_K = 4 + 2     # sigmoid's add and divide, (+ second gate), * x, + out


def se_gate(x, s, prev=None, s2=None, f32=False):
    """-> (out, mag) [N, HW, C]; f32 = the float32 yardstick (stored back to T by the caller)."""
    cv = (lambda t: t.detach().cpu().to(torch.float32)) if f32 else d
    gate = sigmoid_as_kernel(cv(s))
    if s2 is not None:
        gate = gate + sigmoid_as_kernel(cv(s2))
    out = cv(x) * gate.unsqueeze(1)
    mag = out.abs()
    if prev is not None:
        out, mag = out + cv(prev), mag + cv(prev).abs()
    return out, mag


def se_dgate(g, x, s, f32=False):
    """-> (ds, mag) [N, C] = sigmoid'(s) * sum_p g x."""
    cv = (lambda t: t.detach().cpu().to(torch.float32)) if f32 else d
    q = sigmoid_as_kernel(cv(s))
    dot = (cv(g) * cv(x)).sum(1)
    absdot = (cv(g) * cv(x)).abs().sum(1)
    return dot * q * (1.0 - q), absdot * q * (1.0 - q)


# ------------------------------------------------------------------------------------------------ re-arrangements
def parity_to_coarse(x):
    """fine [N, H, W, C] -> coarse [4N, H/2, W/2, C], coarse image 4 n + 2 (y & 1) + (x & 1)."""
    N, H, W, Cn = x.shape
    return torch.stack([x[:, a::2, b::2] for a in (0, 1) for b in (0, 1)], 1).reshape(4 * N, H // 2, W // 2, Cn)


def parity_to_fine(c):
    N4, H2, W2, Cn = c.shape
    c = c.view(N4 // 4, 2, 2, H2, W2, Cn)
    out = torch.zeros(N4 // 4, 2 * H2, 2 * W2, Cn, dtype=c.dtype)
    for a in (0, 1):
        for b in (0, 1):
            out[:, a::2, b::2] = c[:, a, b]
    return out


def mosaic_index(H, W, r):
    hs, ws = -(-H // r), -(-W // r)
    y, x = torch.arange(H), torch.arange(W)
    return 1 + (y % r) * (hs + 1) + y // r, 1 + (x % r) * (ws + 1) + x // r, r * (hs + 1) + 1, r * (ws + 1) + 1


def to_mosaic(x, r):
    N, H, W, Cn = x.shape
    my, mx, MH, MW = mosaic_index(H, W, r)
    m = torch.zeros(N, MH, MW, Cn, dtype=x.dtype)
    m[:, my.view(-1, 1), mx.view(1, -1)] = x
    return m


def from_mosaic(m, H, W, r):
    my, mx, _, _ = mosaic_index(H, W, r)
    return m[:, my.view(-1, 1), mx.view(1, -1)].contiguous()


# ------------------------------------------------------------------------------------------------ depthwise 3x3 (dilation = padding)
def _shift(x, dy, dx):
    """x[n, y + dy, x + dx, c], zero outside."""
    N, H, W, Cn = x.shape
    out = torch.zeros_like(x)
    ys, xs = slice(max(0, -dy), min(H, H - dy)), slice(max(0, -dx), min(W, W - dx))
    if ys.start < ys.stop and xs.start < xs.stop:
        out[:, ys, xs] = x[:, ys.start + dy:ys.stop + dy, xs.start + dx:xs.stop + dx]
    return out


def dw_conv(x, w, dil, flip=False):
    """x [N, H, W, C], w [9, C] -> (out, sumabs): out = sum_t w[flip ? 8 - t : t] x[y + dil (t / 3 - 1), x + dil (t % 3 - 1)]."""
    x, w = d(x), d(w)
    out, sa = torch.zeros_like(x), torch.zeros_like(x)
    for t in range(9):
        sh = _shift(x, dil * (t // 3 - 1), dil * (t % 3 - 1))
        wt = w[8 - t if flip else t]
        out, sa = out + wt * sh, sa + wt.abs() * sh.abs()
    return out, sa


def dw_wgrad(x, gout, dil):
    """-> (dw [9, C], sumabs): dw[t] = sum over pixels of gout * x[y + dil (t / 3 - 1), x + dil (t % 3 - 1)]."""
    x, g = d(x), d(gout)
    dw = torch.stack([(g * _shift(x, dil * (t // 3 - 1), dil * (t % 3 - 1))).sum((0, 1, 2)) for t in range(9)])
    sa = torch.stack([(g.abs() * _shift(x.abs(), dil * (t // 3 - 1), dil * (t % 3 - 1))).sum((0, 1, 2)) for t in range(9)])
    return dw, sa


# ------------------------------------------------------------------------------------------------ depthwise K x K, stride, TF "same" padding
def tf_same(H, K, stride):
    """-> (output extent, top / left padding) of TensorFlow's static "same" rule (efficientnet_pytorch's Conv2dStaticSamePadding)."""
    OH = -(-H // stride)
    return OH, max((OH - 1) * stride + K - H, 0) // 2


def _dwg_windows(x, OH, OW, K, stride, pad):
    """x zero-padded so that window (r, s) of every output is xp[:, r + stride * oy, s + stride * ox]."""
    return F.pad(x, (0, 0, pad, K + stride, pad, K + stride)), [(r, s) for r in range(K) for s in range(K)]


def dwg_fwd(x, w, OH, OW, K, stride, pad):
    """x [N, H, W, C], w [K, K, C] -> (out, sumabs) [N, OH, OW, C]."""
    x, w = d(x), d(w).view(K, K, -1)
    xp, taps = _dwg_windows(x, OH, OW, K, stride, pad)
    ap = xp.abs()
    out = sum(w[r, s] * xp[:, r:r + stride * OH:stride, s:s + stride * OW:stride] for r, s in taps)
    sa = sum(w[r, s].abs() * ap[:, r:r + stride * OH:stride, s:s + stride * OW:stride] for r, s in taps)
    return out, sa


def dwg_bwd_data(gout, w, H, W, K, stride, pad):
    """-> (gin, sumabs, nterms [H, W]): the transpose of dwg_fwd."""
    g, w = d(gout), d(w).view(K, K, -1)
    N, OH, OW, Cn = g.shape
    gp = torch.zeros(N, H + pad + K + stride, W + pad + K + stride, Cn, dtype=REF_DTYPE[0])
    sp, nt = torch.zeros_like(gp), torch.zeros(H + pad + K + stride, W + pad + K + stride, dtype=REF_DTYPE[0])
    for r in range(K):
        for s in range(K):
            gp[:, r:r + stride * OH:stride, s:s + stride * OW:stride] += w[r, s] * g
            sp[:, r:r + stride * OH:stride, s:s + stride * OW:stride] += w[r, s].abs() * g.abs()
            nt[r:r + stride * OH:stride, s:s + stride * OW:stride] += 1
    c = lambda t: t[:, pad:pad + H, pad:pad + W].contiguous()
    return c(gp), c(sp), nt[pad:pad + H, pad:pad + W].contiguous()


def dwg_bwd_w(x, gout, K, stride, pad):
    """-> (dw [K, K, C], sumabs)."""
    x, g = d(x), d(gout)
    OH, OW = g.shape[1], g.shape[2]
    xp, taps = _dwg_windows(x, OH, OW, K, stride, pad)
    dw = torch.stack([(g * xp[:, r:r + stride * OH:stride, s:s + stride * OW:stride]).sum((0, 1, 2)) for r, s in taps]).view(K, K, -1)
    sa = torch.stack([(g.abs() * xp.abs()[:, r:r + stride * OH:stride, s:s + stride * OW:stride]).sum((0, 1, 2)) for r, s in taps]).view(K, K, -1)
    return dw, sa


# ------------------------------------------------------------------------------------------------ BatchNorm + swish sweep (EfficientNet)
BNX_FWD_K = 6 + 2     # fma; sigmoid's add and divide, * z; * dscale; + post
BNX_BWD_K = 8 + 2     # * dscale; fma; sigmoid's add and divide; 1 - sg, * z, 1 +, * sg; * g


def bnx_fwd(y, hw, act, scale=None, shift=None, dscale=None, post=None, f32=False):
    """-> (out, mag) [npix, C]; f32: the float32 yardstick."""
    cv = (lambda t: None if t is None else t.detach().cpu().to(torch.float32)) if f32 else d
    z = cv(y)
    mag = z.abs()
    if scale is not None:
        z, mag = z * cv(scale) + cv(shift), mag * cv(scale).abs() + cv(shift).abs()
    if act == 1:
        sg = sigmoid_as_kernel(z)
        z, mag = z * sg, mag * sg
    if dscale is not None:
        dn = cv(dscale).repeat_interleave(hw).unsqueeze(1)
        z, mag = z * dn, mag * dn.abs()
    if post is not None:
        z, mag = z + cv(post), mag + cv(post).abs()
    return z, mag


def bnx_bwd(g, hw, act, y=None, scale=None, shift=None, dscale=None, f32=False):
    """-> (out, mag): g * dscale[n] * act'(y scale + shift), act' of swish = sg (1 + z (1 - sg))."""
    cv = (lambda t: None if t is None else t.detach().cpu().to(torch.float32)) if f32 else d
    o = cv(g)
    if dscale is not None:
        o = o * cv(dscale).repeat_interleave(hw).unsqueeze(1)
    mag = o.abs()
    if act == 1:
        z = cv(y) * cv(scale) + cv(shift)
        za = cv(y).abs() * cv(scale).abs() + cv(shift).abs()
        sg = sigmoid_as_kernel(z)
        o, mag = o * (sg * (1.0 + z * (1.0 - sg))), mag * (sg * (1.0 + za * (1.0 - sg)))
    return o, mag


# ------------------------------------------------------------------------------------------------ Dice / BCE gradient
DICE_BWD_K = 14 + 2   # sigmoid (2) - t, * scale; exp path: 1 + e (twice), product, divide; dscore: 2 t S, 2 I, -, S S, /; * dpdz, * scale, / C, +


def dice_sums(logits, target):
    """[1 + B, C, 4] float64: I = sum p t, S = sum (p + t), T = sum t, BCE sum; totals over the batch first, then per image."""
    z, t = logits.detach().to(torch.float64), target.detach().to(torch.float64)
    p = torch.sigmoid(z)
    bce = F.binary_cross_entropy_with_logits(z, t, reduction='none')
    per = torch.stack([(p * t).sum(2), (p + t).sum(2), t.sum(2), bce.sum(2)], -1)       # [B, C, 4]
    return torch.cat([per.sum(0, keepdim=True), per], 0)


def dice_bwd(logits, target, sums, loss_kind, grad_scale, f32=False):
    """-> (dL/dz [B, HW, C], mag) from the totals as the kernel reads them (converted to float)."""
    cv = (lambda t: t.detach().cpu().to(torch.float32)) if f32 else d
    z, t = cv(logits), cv(target)
    B, Cn, HW = z.shape
    tot = cv(sums[0].to(torch.float32))
    I, S, T = tot[:, 0].view(1, Cn, 1), tot[:, 1].view(1, Cn, 1), tot[:, 2].view(1, Cn, 1)
    out, mag = torch.zeros_like(z), torch.zeros_like(z)
    if loss_kind != 0:
        sc = grad_scale / (float(B) * float(Cn) * float(HW))
        out, mag = out + (sigmoid_as_kernel(z) - t) * sc, mag + (sigmoid_as_kernel(z) + t.abs()) * abs(sc)
    if loss_kind != 1:
        e = torch.exp(-z.abs())
        dpdz = e / ((1.0 + e) * (1.0 + e))
        big = S > 1e-7
        Ss = torch.where(big, S, torch.ones_like(S))
        dscore = torch.where(big, (2.0 * t * S - 2.0 * I) / (Ss * Ss), 2.0 * t / 1e-7)
        dmag = torch.where(big, (2.0 * t.abs() * S.abs() + 2.0 * I.abs()) / (Ss * Ss), 2.0 * t.abs() / 1e-7)
        live = (T > 0).to(z.dtype)
        out, mag = out + live * (-dscore * dpdz * grad_scale / Cn), mag + live * dmag * dpdz * abs(grad_scale) / Cn
    return out.permute(0, 2, 1).contiguous(), mag.permute(0, 2, 1).contiguous()


# ------------------------------------------------------------------------------------------------ GroupNorm + ReLU (+ bilinear x2)
def gn_stats(y, gamma, beta, G, eps):
    """y [N, HW, C] -> ss [N, C, 2] (scale, shift), stat [N, G, 2] (mean, rstd): biased variance over HW x (C / G)."""
    y = d(y)
    N, HW, Cn = y.shape
    yg = y.view(N, HW, G, Cn // G)
    mean = yg.mean((1, 3))
    var = (yg * yg).mean((1, 3)) - mean * mean
    rstd = 1.0 / torch.sqrt(var.clamp_min(0.0) + eps)
    scale = d(gamma).view(1, Cn) * rstd.repeat_interleave(Cn // G, 1)
    shift = d(beta).view(1, Cn) - mean.repeat_interleave(Cn // G, 1) * scale
    return torch.stack([scale, shift], -1), torch.stack([mean, rstd], -1)


def gn_act(y, ss, H, W, up):
    """relu(y scale + shift) [N, H, W, C], resampled by `up` (bilinear, align_corners) -> (out, mag)."""
    y, ss = d(y), d(ss)
    N, HW, Cn = y.shape
    z = (y * ss[:, None, :, 0] + ss[:, None, :, 1])
    a = torch.where(z < 0, torch.zeros_like(z), z).view(N, H, W, Cn)
    mag = (y.abs() * ss[:, None, :, 0].abs() + ss[:, None, :, 1].abs()).view(N, H, W, Cn)
    if up == 1:
        return a, mag
    return bilinear_resize(a, H * up, W * up)[0], bilinear_resize(mag, H * up, W * up)[0]


def gn_backward(y, g, gamma, ss, stat, G):
    """-> dict(dy, mag, dbeta, dgamma, coef [N, G, 2]) of relu(group_norm(y)) from the forward's ss / stat."""
    y, g, gam, ss, stat = d(y), d(g), d(gamma), d(ss), d(stat)
    N, HW, Cn = y.shape
    cpg = Cn // G
    z = (y * ss[:, None, :, 0] + ss[:, None, :, 1]).to(torch.float32)      # one float fma decides the mask
    dz = torch.where(z > 0, g, torch.zeros_like(g))
    mu, rs = stat[..., 0].repeat_interleave(cpg, 1)[:, None], stat[..., 1].repeat_interleave(cpg, 1)[:, None]
    xh = (y - mu) * rs
    s1, s2 = dz.sum(1), (dz * xh).sum(1)                                   # [N, C]
    cnt = HW * cpg
    m1 = (s1 * gam).view(N, G, cpg).sum(2) / cnt
    m2 = (s2 * gam).view(N, G, cpg).sum(2) / cnt
    M1, M2 = m1.repeat_interleave(cpg, 1)[:, None], m2.repeat_interleave(cpg, 1)[:, None]
    dy = rs * (dz * gam - M1 - xh * M2)
    mag = rs.abs() * (dz.abs() * gam.abs() + M1.abs() + (y.abs() + mu.abs()) * rs.abs() * M2.abs())
    return dict(dy=dy, mag=mag, dbeta=s1.sum(0), dgamma=s2.sum(0), coef=torch.stack([m1, m2], -1))


# ------------------------------------------------------------------------------------------------ squeeze-excite excitation (two FCs)
def _act(h, act):
    return h * sigmoid_as_kernel(h) if act else torch.where(h < 0, torch.zeros_like(h), h)


def _dact(h, act):
    sg = sigmoid_as_kernel(h)
    return sg * (1.0 + h * (1.0 - sg)) if act else (h > 0).to(h.dtype)


def sefc_fwd(m, w1, b1, w2, b2, act, f32=False):
    """-> (s [N, C], h [N, R], mag of s)."""
    cv = (lambda t: t.detach().cpu().to(torch.float32)) if f32 else d
    h = cv(m) @ cv(w1).t() + cv(b1)
    a = _act(h, act)
    return a @ cv(w2).t() + cv(b2), h, a.abs() @ cv(w2).abs().t() + cv(b2).abs()


def sefc_bwd(m, ds, w1, w2, h, act, f32=False):
    """-> dict(dm, dh, dw1, db1, dw2, db2) (+ mags dm_mag, dh_mag)."""
    cv = (lambda t: t.detach().cpu().to(torch.float32)) if f32 else d
    m, ds, w1, w2, h = cv(m), cv(ds), cv(w1), cv(w2), cv(h)
    dh = (ds @ w2) * _dact(h, act)
    return dict(dh=dh, dm=dh @ w1, dw2=ds.t() @ _act(h, act), db2=ds.sum(0), dw1=dh.t() @ m, db1=dh.sum(0),
                dh_mag=(ds.abs() @ w2.abs()) * _dact(h, act).abs(), dm_mag=((ds.abs() @ w2.abs()) * _dact(h, act).abs()) @ w1.abs())
