"""float64 reference of the stem launches behind octseg_stem_op (include/octseg.h; csrc/stem_api.cpp).

The definition, on the NCHW f32 frame [N][3][H][W] and the storage type T:
  frame as seen   normalize: T(f32(f32(raw - mean[c]) * f32(1 / std[c]))), else T(raw); zero outside the frame (conv2d pads the NORMALISED
                  input).  A subtract followed by a multiply cannot be contracted into one operation, so float32 arithmetic on the CPU
                  reproduces the kernels' value bit for bit.
  im2col rows     col[n][oy][ox][(r k + s) 3 + c] = frame as seen at (2 oy - pad + r, 2 ox - pad + s), channel c; columns >= 3 k^2 are zero
  weights         the fp32 arena weight [64][160], k = (r 7 + s) 3 + c (times wscale[o] in f32 for the eval fold) rounded to T
  y               conv 7x7 stride 2 pad 3 of the two (+ bias, relu_out): the f32 value; stored as T(y) -- thin.hip's 'direct' rule, no accumulate
  statistics      sum y and sum y^2 of that f32 value over all pixels
  weight gradient dW[o][k] = old + sum over pixels of dy[n][oy][ox][o] col[n][oy][ox][k]; columns 147..159 keep what they held
Everything is evaluated in sweep_ref.REF_DTYPE[0], as tests/conv_ref.py does.
"""
import torch
import torch.nn.functional as F

import conv_ref as CR
import sweep_ref as R

KTAPS = 147


def frame_as_seen(stem, t, T):
    """[N][3][H][W] in the reference dtype."""
    x = t['img'].detach().cpu().to(torch.float32)
    if stem.normalize:
        mean = torch.tensor(stem.mean, dtype=torch.float32).view(1, 3, 1, 1)
        inv = (torch.ones(3, dtype=torch.float32) / torch.tensor(stem.std, dtype=torch.float32)).view(1, 3, 1, 1)
        x = (x - mean) * inv          # two float32 operations, each rounded once
    return x.to(T).to(R.REF_DTYPE[0])


def im2col(stem, t, T):
    """[N][OH][OW][KP] in the reference dtype (every value a T)."""
    k, p = stem.ksize, stem.pad
    oh, ow = stem.out_hw
    x = frame_as_seen(stem, t, T)
    xp = F.pad(x, (p, k, p, k))       # (more than enough right / bottom: the slices below never reach the end)
    col = torch.zeros((stem.N, oh, ow, stem.KP), dtype=x.dtype)
    for r in range(k):
        for s in range(k):
            for c in range(3):
                col[..., (r * k + s) * 3 + c] = xp[:, c, r:r + 2 * oh:2, s:s + 2 * ow:2]
    return col


def weight_as_seen(t, T):
    """[64][3][7][7] in the reference dtype."""
    w = t['w'].detach().cpu().to(torch.float32)
    if t.get('wscale') is not None:
        w = w * t['wscale'].detach().cpu().to(torch.float32).view(-1, 1)      # one float32 multiply, as thin.hip does it
    w = w.to(T).to(R.REF_DTYPE[0])
    return w[:, :KTAPS].reshape(64, 7, 7, 3).permute(0, 3, 1, 2).contiguous()


def forward_f32value(stem, t, T):
    """y [N][64][OH][OW]: the value the epilogue holds in f32."""
    y = F.conv2d(frame_as_seen(stem, t, T), weight_as_seen(t, T), stride=2, padding=3)
    if t.get('bias') is not None:
        y = y + CR.ref(t['bias']).view(1, -1, 1, 1)
    if stem.relu_out:
        y = y.clamp_min(0)
    return y


def forward(stem, t, T):
    """Expected y (NHWC, T-representable), stats [64][2] = the slab rows' sum (with a slab), yf = the f32 value."""
    y = forward_f32value(stem, t, T)
    out = {'y': CR.nhwc(CR.rnd(y, T)), 'yf': y}
    if t.get('slab') is not None:
        out['stats'] = torch.stack([y.sum(dim=(0, 2, 3)), (y * y).sum(dim=(0, 2, 3))], dim=1)
    return out


def backward_weight_terms(stem, t, T, absolute=False):
    """dW [64][160] of the pass alone (absolute: every product replaced by its absolute value: the Rule R yardstick)."""
    dy = CR.ref(t['dy'])
    col = im2col(stem, t, T)
    if absolute:
        dy, col = dy.abs(), col.abs()
    return torch.einsum('nyxo,nyxk->ok', dy, col)


def backward_weight(stem, t, T):
    return {'dW': CR.ref(t['dW']) + backward_weight_terms(stem, t, T)}
