"""float64 reference of one conv layer pass with its fused operand and epilogue paths, and the guarded buffers of its single-launch tests.

The definition (include/octseg.h, octseg_conv_layer_op; csrc/kernels.h for the store rules), on NHWC tensors of the storage type T:
  virtual input   per source: relu?(x * scale + shift) rounded to T, nearest x2 where `up`; sources concatenated along C; the zero padding is
                  applied AFTER the affine (a padding pixel is 0, not relu(shift))
  weights         the fp32 arena weight [R][S][O][I] (times wscale[o] in f32 for the eval fold) rounded to T
  y               conv / ConvTranspose2d(k4, s2, p1) of the two, + bias, relu_out: the f32 value
  statistics      sum y and sum y^2 of that f32 value (before the storage rounding, bias included) over the pixels inside the map
  store           T(y); accum: T(T(y) + old) ('staged' routes: conv_mfma, gemm1x1, conv3x3p) or T(y + old) ('direct': thin.hip);
                  pool: T(old + T(q00) + T(q01) + T(q10) + T(q11)) (staged) or T(old + q00 + q01 + q10 + q11) (direct); head: the f32 y as NCHW
  gradients       of the same definition: dgrad per destination slice, wgrad over the virtual input (accumulated onto dW)
Everything is evaluated in REF_DTYPE[0] (sweep_ref.as_float32 switches it to float32 for the exactness proofs of tests/test_convops.py).
`wrong` deliberately breaks the definition ('pad_affine': the padding receives the affine; 'stats_rounded': statistics of the rounded
value) so that the CPU tests can show that the cases tell the difference.
"""
import torch
import torch.nn.functional as F

import sweep_ref as R

POISON = 3.0 * 2 ** 14     # finite, exact in bf16 / f16 / f32, gross next to operands below 12: a halo read that leaks into a sum shows


def ref(t):
    return t.detach().cpu().to(R.REF_DTYPE[0])


def rnd(v, T):
    """A value of the reference dtype rounded to T (through float32: the value must be a float32 already when T is narrower)."""
    f = v.to(torch.float32)
    if T != torch.float32 and R.REF_DTYPE[0] == torch.float64:
        assert torch.equal(f.to(torch.float64), v), 'a value to be rounded to T is not exact in float32'
    return f.to(T).to(R.REF_DTYPE[0])


def nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


def virtual_input(layer, t, T, wrong=None):
    """[N][Cin][H + 2 pad][W + 2 pad]: the concatenated input as the kernels see it, padding included."""
    p = 0 if layer.transposed else layer.pad
    parts = []
    for i, s in enumerate(layer.srcs):
        x = nchw(ref(t[f'x{i}']))
        fill = torch.zeros(s.C, dtype=x.dtype)
        if s.affine:
            sc, sh = ref(t[f'scale{i}']).view(1, -1, 1, 1), ref(t[f'shift{i}']).view(1, -1, 1, 1)
            x = x * sc + sh
            fill = sh.reshape(-1).clone()
            if s.relu:
                x, fill = x.clamp_min(0), fill.clamp_min(0)
            x, fill = rnd(x, T), rnd(fill, T)
        if s.up:
            x = x.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)
        xp = torch.zeros((x.shape[0], s.C, layer.H + 2 * p, layer.W + 2 * p), dtype=x.dtype)
        if wrong == 'pad_affine':
            xp += fill.view(1, -1, 1, 1)
        xp[:, :, p:p + layer.H, p:p + layer.W] = x
        parts.append(xp)
    return torch.cat(parts, dim=1)


def weight_as_seen(layer, t, T, fold=True):
    """[R][S][O][I] in the reference dtype: the arena weight (times wscale in float32) rounded to T."""
    w = t['w'].detach().cpu().to(torch.float32)
    if fold and t.get('wscale') is not None:
        w = w * t['wscale'].detach().cpu().to(torch.float32).view(1, 1, -1, 1)      # one float32 multiply, as the packer does it
    return w.to(T).to(R.REF_DTYPE[0])


def conv_of(layer, xp, w):
    if layer.transposed:
        return F.conv_transpose2d(xp, w.permute(3, 2, 0, 1).contiguous(), stride=2, padding=1)
    return F.conv2d(xp, w.permute(2, 3, 0, 1).contiguous(), stride=layer.stride)


def forward_f32value(layer, t, T, wrong=None):
    """y [N][Cout][OH][OW]: the value the epilogue holds in f32 (bias added, relu_out applied)."""
    y = conv_of(layer, virtual_input(layer, t, T, wrong), weight_as_seen(layer, t, T))
    if t.get('bias') is not None:
        y = y + ref(t['bias']).view(1, -1, 1, 1)
    if layer.relu_out:
        y = y.clamp_min(0)
    return y


def store(y, old, T, accum, rule):
    """NCHW f32 value -> what the destination holds (reference dtype, T-representable)."""
    if not accum:
        return rnd(y, T)
    return rnd(rnd(y, T) + old, T) if rule == 'staged' else rnd(y + old, T)


def pool_store(y, old, T, accum, rule):
    q = rnd(y, T) if rule == 'staged' else y
    s = q[:, :, 0::2, 0::2] + q[:, :, 0::2, 1::2] + q[:, :, 1::2, 0::2] + q[:, :, 1::2, 1::2]
    return rnd(s + old if accum else s, T)


def forward(layer, t, T, rule, wrong=None):
    """Expected tensors of a forward: y (NHWC T, or NCHW f32 in head mode), stats [Cout][2] = the slab rows' sum (None without a slab)."""
    y = forward_f32value(layer, t, T, wrong)
    out = {}
    if layer.head:
        out['y'] = y
    else:
        old = nchw(ref(t['y'])) if layer.accum[0] else None
        out['y'] = nhwc(store(y, old, T, layer.accum[0], rule))
    if t.get('slab') is not None:
        ys = rnd(y, T) if wrong == 'stats_rounded' else y
        out['stats'] = torch.stack([ys.sum(dim=(0, 2, 3)), (ys * ys).sum(dim=(0, 2, 3))], dim=1)
    out['yf'] = y
    return out


def backward_data_full(layer, t, T):
    """dL/d(virtual input) [N][Cin][H][W] in f32-value form."""
    dy = nchw(ref(t['dy']))
    w = weight_as_seen(layer, t, T, fold=False)
    if layer.transposed:      # the gradient of a ConvTranspose2d is the plain conv with the same kernel
        return F.conv2d(dy, w.permute(3, 2, 0, 1).contiguous(), stride=2, padding=1)
    oh, ow = layer.out_hw
    oph = layer.H - ((oh - 1) * layer.stride - 2 * layer.pad + layer.R)
    opw = layer.W - ((ow - 1) * layer.stride - 2 * layer.pad + layer.R)
    return F.conv_transpose2d(dy, w.permute(2, 3, 0, 1).contiguous(), stride=layer.stride, padding=layer.pad, output_padding=(oph, opw))


def backward_data(layer, t, T, rule):
    """Expected dx{i} (NHWC T) per destination."""
    g = backward_data_full(layer, t, T)
    out, c0 = {'gf': g}, 0
    for i, s in enumerate(layer.srcs):
        gi = g[:, c0:c0 + s.C]
        old = nchw(ref(t[f'dx{i}'])) if layer.accum[i] else None
        out[f'dx{i}'] = nhwc(pool_store(gi, old, T, layer.accum[i], rule) if layer.pool[i] else store(gi, old, T, layer.accum[i], rule))
        c0 += s.C
    return out


def backward_weight_terms(layer, t, T, absolute=False):
    """dW [R][S][O][I] of the pass alone (absolute: every product replaced by its absolute value: the Rule R yardstick)."""
    dy = nchw(ref(t['dy']))
    xp = virtual_input(layer, t, T)
    if absolute:
        dy, xp = dy.abs(), xp.abs()
    Rk, O, I = layer.R, layer.Cout, layer.Cin
    dW = torch.zeros((Rk, Rk, O, I), dtype=dy.dtype)
    if layer.transposed:      # y[oy] += x[iy] w[r] with oy = 2 iy - 1 + r
        dyp = F.pad(dy, (1, 2, 1, 2))
        for r in range(4):
            for s in range(4):
                dW[r, s] = torch.einsum('noyx,niyx->oi', dyp[:, :, r:r + 2 * layer.H:2, s:s + 2 * layer.W:2], xp)
        return dW
    oh, ow = layer.out_hw
    st = layer.stride
    for r in range(Rk):
        for s in range(Rk):
            dW[r, s] = torch.einsum('noyx,niyx->oi', dy, xp[:, :, r:r + st * (oh - 1) + 1:st, s:s + st * (ow - 1) + 1:st])
    return dW


def backward_weight(layer, t, T):
    return {'dW': ref(t['dW']) + backward_weight_terms(layer, t, T)}


# ------------------------------------------------------------------------------------------------ exactness
def lowbit(v):
    """Largest power of two that divides every element of v (float64 tensor of dyadic values); 0 values are skipped."""
    v = v.to(torch.float64).abs().reshape(-1)
    v = v[v > 0]
    if v.numel() == 0:
        return 1.0
    g = 1.0
    while not bool(torch.equal((v / g).round(), v / g)):
        g /= 2
    while bool(torch.equal((v / (2 * g)).round(), v / (2 * g))):
        g *= 2
    return g


def product_granularity(layer, t, T):
    """Power of two that every product (activation as seen x weight as seen) and the bias are a multiple of."""
    with torch.no_grad():
        g = lowbit(virtual_input(layer, t, T).to(torch.float64)) * lowbit(weight_as_seen(layer, t, T).to(torch.float64))
        if t.get('bias') is not None:
            g = min(g, lowbit(t['bias']))
    return g


# ------------------------------------------------------------------------------------------------ guarded buffers
class Guard(R.Guard):
    """sweep_ref.Guard plus inputs between margins of a large finite poison (3 * 2^14 in the tensor's own type): a halo read that leaves the
    tensor then shows in the sums as a gross error instead of a NaN that a masked lane might swallow.  check() covers both kinds."""

    def __init__(self, device):
        super().__init__(device)
        self.poisoned = []

    def put_poisoned(self, t):
        if t is None:
            return None
        esz = t.element_size()
        n = t.numel()
        m = R.MARGIN // esz
        buf = torch.full((m + (n + 15) // 16 * 16 + m,), POISON, dtype=t.dtype, device=self.device)
        assert buf.data_ptr() % 16 == 0 and (m * esz) % 16 == 0
        view = buf[m:m + n].view(*t.shape)
        view.copy_(t)
        self.poisoned.append((buf, m, n))
        return view

    def check(self):
        super().check()
        for buf, m, n in self.poisoned:
            assert bool((buf[:m] == POISON).all()) and bool((buf[m + n:] == POISON).all()), 'a kernel wrote into the margin of an input'
