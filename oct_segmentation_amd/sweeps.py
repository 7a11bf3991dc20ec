"""Single-op bindings of the NHWC sweep kernels (BatchNorm finalize / apply / backward, pools, resamplers,
gates, gradient plumbing) over ``octseg_sweep_op``.

Like ``ops.py`` they exist so that each HIP kernel can be pinned against a float64 reference alone
(tests/test_gpu_sweeps.py); the network path reaches the same launchers through the plan.  One call is one
launcher.  Every wrapper derives the extent of every buffer from the shapes it is given and checks the
tensors against it before the call, so that a call can not reach outside its tensors; the library checks
alignment, vector widths, dtypes and null pointers and refuses with a status (``sweep_op_raw`` returns it).
"""
import ctypes as C

import torch

from . import _lib as L
from .ops import _dt

# order of the `octseg_sweep` enum in include/octseg.h
OP_NAMES = ('bn_finalize_train', 'bn_finalize_small', 'bn_finalize_eval', 'bn_finalize_frozen', 'bn_act', 'bn_bwd_small', 'bn_bwd_reduce',
            'bn_bwd_finalize', 'bn_bwd_apply', 'masked_accum', 'pool2x2_accum', 'up2_fill', 'relu', 'add2', 'drop_elem', 'merge_drop',
            'drop_bwd', 'channel_sum', 'tensor_stats', 'maxpool_fwd', 'maxpool_bwd_idx', 'bilinear_resize', 'bilinear_resize_adjoint',
            'bilinear_adjoint', 'bin_mean', 'bin_mean_bwd', 'image_sum', 'image_bcast', 'se_gate', 'se_dgate', 'parity_permute', 'mosaic',
            'dw_conv', 'dw_wgrad', 'cam_seed', 'dwg_fwd', 'dwg_bwd_data', 'dwg_bwd_w', 'bnx_fwd', 'bnx_bwd', 'dice_bwd',
            'gn_forward', 'gn_backward', 'sefc_fwd', 'sefc_bwd')
OPS = {n: i for i, n in enumerate(OP_NAMES)}
SLAB_PART_DOUBLES = 2 * 16384   # `part` scratch of the slab reductions
SLAB_COUNTERS = 64              # zeroed uint32 tickets


def sweep_op_raw(op, dtype, ptrs, iargs, fargs=(), stream=None):
    """The bare call: ptrs are integer addresses (or None).  Returns the library's status code."""
    n = len(ptrs)
    pa = (C.c_void_p * max(n, 1))(*ptrs)
    ia = (C.c_longlong * max(len(iargs), 1))(*[int(v) for v in iargs])
    fa = (C.c_double * max(len(fargs), 1))(*[float(v) for v in fargs])
    return L.lib().octseg_sweep_op(OPS[op] if isinstance(op, str) else op, dtype, pa, n, ia, len(iargs), fa, len(fargs), stream)


def _call(op, dtype, tensors, iargs, fargs=()):
    for t in tensors:
        assert t is None or (t.is_cuda and t.is_contiguous()), f'{op}: contiguous cuda tensors expected'
    L.check(sweep_op_raw(op, dtype, [None if t is None else t.data_ptr() for t in tensors], iargs, fargs, L.stream_ptr()))


def _need(t, numel, dtype, what, optional=False):
    if t is None:
        assert optional, f'{what} is required'
        return
    assert t.dtype == dtype, f'{what}: {t.dtype}, expected {dtype}'
    assert t.numel() == numel, f'{what}: {t.numel()} elements, expected {numel}'


def _f32(t, numel, what, optional=False):
    _need(t, numel, torch.float32, what, optional)


def _scratch(part, counters):
    assert part.dtype == torch.float64 and part.numel() >= SLAB_PART_DOUBLES, 'part: float64[32768] scratch'
    assert counters.dtype == torch.int32 and counters.numel() >= SLAB_COUNTERS, 'counters: 64 zeroed int32 tickets'


def se_dgate_shares(HW):
    return min(max(HW // 64, 1), 64)


# ---------------------------------------------------------------- BatchNorm finalize
def bn_finalize_train(slab, count, gamma, beta, running_mean, running_var, momentum, eps, scale, shift, mean, rstd, part, counters,
                      dtype=L.F32):
    rows, Cn = slab.shape[0], slab.shape[1]
    _f32(slab, rows * Cn * 2, 'slab')
    for n, t in (('gamma', gamma), ('beta', beta), ('running_mean', running_mean), ('running_var', running_var), ('scale', scale),
                 ('shift', shift), ('mean', mean), ('rstd', rstd)):
        _f32(t, Cn, n)
    _scratch(part, counters)
    _call('bn_finalize_train', dtype, [slab, gamma, beta, running_mean, running_var, scale, shift, mean, rstd, part, counters], [rows, Cn],
          [count, momentum, eps])


def bn_finalize_small(y, gamma, beta, running_mean, running_var, momentum, eps, scale, shift, mean, rstd, dtype=None):
    count, Cn = y.shape
    for n, t in (('gamma', gamma), ('beta', beta), ('running_mean', running_mean), ('running_var', running_var), ('scale', scale),
                 ('shift', shift), ('mean', mean), ('rstd', rstd)):
        _f32(t, Cn, n)
    _call('bn_finalize_small', _dt(y) if dtype is None else dtype, [y, gamma, beta, running_mean, running_var, scale, shift, mean, rstd],
          [count, Cn], [momentum, eps])


def bn_finalize_eval(gamma, beta, running_mean, running_var, eps, scale, shift, dtype=L.F32):
    Cn = gamma.numel()
    for n, t in (('gamma', gamma), ('beta', beta), ('running_mean', running_mean), ('running_var', running_var), ('scale', scale), ('shift', shift)):
        _f32(t, Cn, n)
    _call('bn_finalize_eval', dtype, [gamma, beta, running_mean, running_var, scale, shift], [Cn], [eps])


def bn_finalize_frozen(gamma, beta, running_mean, running_var, eps, scale, shift, mean, rstd, coef, dtype=L.F32):
    Cn = gamma.numel()
    for n, t in (('gamma', gamma), ('beta', beta), ('running_mean', running_mean), ('running_var', running_var), ('scale', scale),
                 ('shift', shift), ('mean', mean), ('rstd', rstd)):
        _f32(t, Cn, n)
    _f32(coef, 2 * Cn, 'coef')
    _call('bn_finalize_frozen', dtype, [gamma, beta, running_mean, running_var, scale, shift, mean, rstd, coef], [Cn], [eps])


# ---------------------------------------------------------------- BatchNorm apply / backward
def bn_act(y, out, scale=None, shift=None, res=None, rscale=None, rshift=None, post=None, relu=False, maskbits=None, dtype=None):
    """y, res, post, out: [npix, C] tensors of one dtype; maskbits: uint8, one byte per 16-byte vector."""
    npix, Cn = y.shape
    dt = _dt(y) if dtype is None else dtype
    vec = 4 if y.dtype == torch.float32 else 8
    for n, t in (('res', res), ('post', post)):
        _need(t, npix * Cn, y.dtype, n, optional=True)
    _need(out, npix * Cn, y.dtype, 'out')
    for n, t in (('scale', scale), ('shift', shift), ('rscale', rscale), ('rshift', rshift)):
        _f32(t, Cn, n, optional=True)
    if maskbits is not None:
        assert Cn % vec == 0
        _need(maskbits, npix * (Cn // vec), torch.uint8, 'maskbits')
    _call('bn_act', dt, [y, scale, shift, res, rscale, rshift, post, out, maskbits], [npix, Cn, int(relu)])


def _bn_bwd(op, dt, npix, Cn, mask, rows, res_store, g=None, y=None, out=None, maskbits=None, scale=None, shift=None, mean=None, rstd=None,
            gamma=None, slab=None, dgamma=None, dbeta=None, coef=None, dy=None, part=None, counters=None, res_grad=None):
    T = torch.float32 if dt == L.F32 else (torch.bfloat16 if dt == L.BF16 else torch.float16)
    vec = 4 if dt == L.F32 else 8
    for n, t in (('g', g), ('y', y), ('out', out), ('dy', dy), ('res_grad', res_grad)):
        _need(t, npix * Cn, T, n, optional=True)
    if maskbits is not None:
        assert Cn % vec == 0
        _need(maskbits, npix * (Cn // vec), torch.uint8, 'maskbits')
    for n, t in (('scale', scale), ('shift', shift), ('mean', mean), ('rstd', rstd), ('gamma', gamma), ('dgamma', dgamma), ('dbeta', dbeta)):
        _f32(t, Cn, n, optional=True)
    _f32(coef, 2 * Cn, 'coef', optional=True)
    _f32(slab, rows * Cn * 2, 'slab', optional=True)
    if part is not None or counters is not None:
        _scratch(part, counters)
    _call(op, dt, [g, y, out, maskbits, scale, shift, mean, rstd, gamma, slab, dgamma, dbeta, coef, dy, part, counters, res_grad],
          [npix, Cn, mask, rows, int(res_store)])


def bn_bwd_small(g, y, scale, shift, mean, rstd, gamma, dgamma, dbeta, coef, dy, mask=0, out=None, maskbits=None, res_grad=None,
                 res_store=False, dtype=None):
    npix, Cn = y.shape
    _bn_bwd('bn_bwd_small', _dt(y) if dtype is None else dtype, npix, Cn, mask, 1, res_store, g=g, y=y, out=out, maskbits=maskbits,
            scale=scale, shift=shift, mean=mean, rstd=rstd, gamma=gamma, dgamma=dgamma, dbeta=dbeta, coef=coef, dy=dy, res_grad=res_grad)


def bn_bwd_reduce(g, y, scale, shift, mean, rstd, slab, mask=0, out=None, maskbits=None, dtype=None):
    npix, Cn = y.shape
    _bn_bwd('bn_bwd_reduce', _dt(y) if dtype is None else dtype, npix, Cn, mask, slab.shape[0], False, g=g, y=y, out=out, maskbits=maskbits,
            scale=scale, shift=shift, mean=mean, rstd=rstd, slab=slab)


def bn_bwd_finalize(slab, npix, dgamma, dbeta, coef, part, counters, dtype=L.F32):
    rows, Cn = slab.shape[0], slab.shape[1]
    _bn_bwd('bn_bwd_finalize', dtype, npix, Cn, 0, rows, False, slab=slab, dgamma=dgamma, dbeta=dbeta, coef=coef, part=part, counters=counters)


def bn_bwd_apply(g, y, scale, shift, mean, rstd, gamma, coef, dy, mask=0, out=None, maskbits=None, res_grad=None, res_store=False, dtype=None):
    npix, Cn = y.shape
    _bn_bwd('bn_bwd_apply', _dt(y) if dtype is None else dtype, npix, Cn, mask, 1, res_store, g=g, y=y, out=out, maskbits=maskbits,
            scale=scale, shift=shift, mean=mean, rstd=rstd, gamma=gamma, coef=coef, dy=dy, res_grad=res_grad)


# ---------------------------------------------------------------- gradient plumbing and plain element-wise sweeps
def masked_accum(dst, g, out_mask=None, store=False, dtype=None):
    n = g.numel()
    _need(dst, n, g.dtype, 'dst')
    _need(out_mask, n, g.dtype, 'out_mask', optional=True)
    _call('masked_accum', _dt(g) if dtype is None else dtype, [dst, g, out_mask], [n, int(store)])


def pool2x2_accum(dst, src, store=False, dtype=None):
    N, H, W, Cn = dst.shape
    _need(src, N * 4 * H * W * Cn, dst.dtype, 'src')
    _call('pool2x2_accum', _dt(dst) if dtype is None else dtype, [dst, src], [N, H, W, Cn, int(store)])


def up2_fill(x, out):
    N, H, W, Cn = x.shape
    _need(out, N * 4 * H * W * Cn, x.dtype, 'out')
    _call('up2_fill', _dt(x), [x, out], [N, H, W, Cn])


def relu(x, out, mask=None):
    _need(out, x.numel(), x.dtype, 'out')
    _need(mask, x.numel(), x.dtype, 'mask', optional=True)
    _call('relu', _dt(x), [x, mask, out], [x.numel()])


def add2(a, b, out):
    _need(b, a.numel(), a.dtype, 'b')
    _need(out, a.numel(), a.dtype, 'out')
    _call('add2', _dt(a), [a, b, out], [a.numel()])


def drop_elem(x, out, keep=None, mscale=1.0):
    _need(out, x.numel(), x.dtype, 'out')
    _f32(keep, x.numel(), 'keep', optional=True)
    _call('drop_elem', _dt(x), [x, keep, out], [x.numel()], [mscale])


def merge_drop(a0, a1, a2, a3, out, m=None, mscale=1.0):
    N, HW, Cn = a0.shape
    for n, t in (('a1', a1), ('a2', a2), ('a3', a3), ('out', out)):
        _need(t, N * HW * Cn, a0.dtype, n)
    _f32(m, N * Cn, 'm', optional=True)
    _call('merge_drop', _dt(a0), [a0, a1, a2, a3, m, out], [N, HW, Cn], [mscale])


def drop_bwd(gout, gin, m=None, mscale=1.0):
    N, HW, Cn = gout.shape
    _need(gin, N * HW * Cn, gout.dtype, 'gin')
    _f32(m, N * Cn, 'm', optional=True)
    _call('drop_bwd', _dt(gout), [gout, m, gin], [N, HW, Cn], [mscale])


def channel_sum(g, Cn, out, dtype=None):
    """g: [npix, Cstride]; out[c] += sum over the pixels of g[:, c] for c < Cn."""
    npix, Cstride = g.shape
    assert 1 <= Cn <= Cstride
    _f32(out, Cn, 'out')
    _call('channel_sum', _dt(g) if dtype is None else dtype, [g, out], [npix, Cstride, Cn])


def tensor_stats(y, slab, dtype=None):
    npix, Cn = y.shape
    rows = slab.shape[0]
    _f32(slab, rows * Cn * 2, 'slab')
    _call('tensor_stats', _dt(y) if dtype is None else dtype, [y, slab], [npix, Cn, rows])


# ---------------------------------------------------------------- pools and resamplers
def maxpool_fwd(x, out, idx=None):
    N, H, W, Cn = x.shape
    _need(out, N * (H // 2) * (W // 2) * Cn, x.dtype, 'out')
    _need(idx, N * (H // 2) * (W // 2) * Cn, torch.uint8, 'idx', optional=True)
    _call('maxpool_fwd', _dt(x), [x, out, idx], [N, H, W, Cn])


def maxpool_bwd_idx(idx, gout, gin, store=True, dtype=None):
    N, H, W, Cn = gin.shape
    _need(gout, N * (H // 2) * (W // 2) * Cn, gin.dtype, 'gout')
    _need(idx, N * (H // 2) * (W // 2) * Cn, torch.uint8, 'idx')
    _call('maxpool_bwd_idx', _dt(gin) if dtype is None else dtype, [idx, gout, gin], [N, H, W, Cn, int(store)])


def bilinear_resize(x, out):
    N, IH, IW, Cn = x.shape
    assert out.dim() == 4 and out.shape[0] == N and out.shape[3] == Cn and out.dtype == x.dtype
    _call('bilinear_resize', _dt(x), [x, out], [N, IH, IW, out.shape[1], out.shape[2], Cn])


def bilinear_resize_adjoint(gout, gin, dtype=None):
    N, IH, IW, Cn = gin.shape
    assert gout.dim() == 4 and gout.shape[0] == N and gout.shape[3] == Cn and gout.dtype == gin.dtype
    _call('bilinear_resize_adjoint', _dt(gin) if dtype is None else dtype, [gout, gin], [N, IH, IW, gout.shape[1], gout.shape[2], Cn])


def bilinear_adjoint(gout, gin, up, dtype=None):
    N, H, W, Cn = gin.shape
    _need(gout, N * H * up * W * up * Cn, gin.dtype, 'gout')
    _call('bilinear_adjoint', _dt(gin) if dtype is None else dtype, [gout, gin], [N, H, W, Cn, up])


def bin_mean(x, out, k):
    N, H, W, Cn = x.shape
    _need(out, N * k * k * Cn, x.dtype, 'out')
    _call('bin_mean', _dt(x), [x, out], [N, H, W, Cn, k])


def bin_mean_bwd(gout, gin, k, accum=False, dtype=None):
    N, H, W, Cn = gin.shape
    _need(gout, N * k * k * Cn, gin.dtype, 'gout')
    _call('bin_mean_bwd', _dt(gin) if dtype is None else dtype, [gout, gin], [N, H, W, Cn, k, int(accum)])


# ---------------------------------------------------------------- per-image vectors and gates
def image_sum(x, out, div=1.0):
    N, HW, Cn = x.shape
    _need(out, N * Cn, x.dtype, 'out')
    _call('image_sum', _dt(x), [x, out], [N, HW, Cn], [div])


def image_bcast(v, out, scale=1.0, accum=False):
    N, HW, Cn = out.shape
    _need(v, N * Cn, out.dtype, 'in')
    _call('image_bcast', _dt(out), [v, out], [N, HW, Cn, int(accum)], [scale])


def se_gate(x, s, out, accum=False, s2=None):
    N, HW, Cn = x.shape
    _need(s, N * Cn, x.dtype, 's')
    _need(s2, N * Cn, x.dtype, 's2', optional=True)
    _need(out, N * HW * Cn, x.dtype, 'out')
    _call('se_gate', _dt(x), [x, s, out, s2], [N, HW, Cn, int(accum)])


def se_dgate(g, x, s, ds, part, s2=None, ds2=None, dtype=None):
    N, HW, Cn = x.shape
    _need(g, N * HW * Cn, x.dtype, 'g')
    for n, t in (('s', s), ('ds', ds)):
        _need(t, N * Cn, x.dtype, n)
    for n, t in (('s2', s2), ('ds2', ds2)):
        _need(t, N * Cn, x.dtype, n, optional=True)
    _f32(part, N * se_dgate_shares(HW) * Cn, 'part')
    _call('se_dgate', _dt(x) if dtype is None else dtype, [g, x, s, ds, part, s2, ds2], [N, HW, Cn])


# ---------------------------------------------------------------- re-arrangements
def parity_permute(src, dst, N, H, W, to_coarse, accum=False):
    """fine [N, H, W, C] <-> coarse [4N, H/2, W/2, C]; N, H, W describe the fine tensor."""
    Cn = src.shape[-1]
    _need(src, N * H * W * Cn, dst.dtype, 'src')
    _need(dst, N * H * W * Cn, src.dtype, 'dst')
    _call('parity_permute', _dt(src), [src, dst], [N, H, W, Cn, int(to_coarse), int(accum)])


def mosaic_extent(H, W, r):
    hs, ws = -(-H // r), -(-W // r)
    return r * (hs + 1) + 1, r * (ws + 1) + 1


def mosaic(src, dst, N, H, W, r, to_mosaic, accum=False):
    Cn = src.shape[-1]
    MH, MW = mosaic_extent(H, W, r)
    fine, mos = (src, dst) if to_mosaic else (dst, src)
    _need(fine, N * H * W * Cn, src.dtype, 'fine tensor')
    _need(mos, N * MH * MW * Cn, src.dtype, 'mosaic tensor')
    _call('mosaic', _dt(src), [src, dst], [N, H, W, Cn, r, int(to_mosaic), int(accum)])


# ---------------------------------------------------------------- depthwise 3x3 on channel slices, the CAM seed
def dw_conv(x, ic0, out, oc0, w, wc0, Cn, dil, flip=False, accum=False):
    """out[..., oc0:oc0 + Cn] (+)= depthwise 3x3 (dilation = padding = dil) of x[..., ic0:ic0 + Cn] with w[:, wc0:wc0 + Cn]; w: f32 [9, wC]."""
    N, H, W, inC = x.shape
    assert out.dim() == 4 and tuple(out.shape[:3]) == (N, H, W) and out.dtype == x.dtype and w.dim() == 2 and w.shape[0] == 9
    assert 0 <= ic0 and ic0 + Cn <= inC and 0 <= oc0 and oc0 + Cn <= out.shape[3] and 0 <= wc0 and wc0 + Cn <= w.shape[1]
    _f32(w, 9 * w.shape[1], 'w')
    _call('dw_conv', _dt(x), [x, out, w], [inC, ic0, out.shape[3], oc0, w.shape[1], wc0, N, H, W, Cn, dil, int(flip), int(accum)])


def dw_wgrad(x, ic0, gout, oc0, dw, wc0, Cn, dil, dtype=None):
    N, H, W, inC = x.shape
    assert gout.dim() == 4 and tuple(gout.shape[:3]) == (N, H, W) and gout.dtype == x.dtype and dw.dim() == 2 and dw.shape[0] == 9
    assert 0 <= ic0 and ic0 + Cn <= inC and 0 <= oc0 and oc0 + Cn <= gout.shape[3] and 0 <= wc0 and wc0 + Cn <= dw.shape[1]
    _f32(dw, 9 * dw.shape[1], 'dw')
    _call('dw_wgrad', _dt(x) if dtype is None else dtype, [x, gout, dw], [inC, ic0, gout.shape[3], oc0, dw.shape[1], wc0, N, H, W, Cn, dil])


def cam_seed(seed, dlogits, dtype=None):
    """seed: f32 [B, C, HW] -> dlogits: T [B, HW, CP], zeros beyond C."""
    B, Cn, HW = seed.shape
    _f32(seed, B * Cn * HW, 'seed')
    assert dlogits.dim() == 3 and tuple(dlogits.shape[:2]) == (B, HW) and dlogits.shape[2] >= Cn
    _call('cam_seed', _dt(dlogits) if dtype is None else dtype, [seed, dlogits], [B, Cn, HW, dlogits.shape[2]])


# ---------------- depthwise K x K with stride and TF "same" padding, the BatchNorm + swish sweep, the Dice gradient
def _dwg_shapes(fine, coarse, w, K):
    N, H, W, Cn = fine.shape
    assert coarse.dim() == 4 and coarse.shape[0] == N and coarse.shape[3] == Cn and coarse.dtype == fine.dtype
    _f32(w, K * K * Cn, 'w')
    return [N, H, W, Cn, coarse.shape[1], coarse.shape[2], K]


def dwg_fwd(x, out, w, K, stride, pad):
    _call('dwg_fwd', _dt(x), [x, out, w], _dwg_shapes(x, out, w, K) + [stride, pad])


def dwg_bwd_data(gout, gin, w, K, stride, pad, accum=False, dtype=None):
    _call('dwg_bwd_data', _dt(gin) if dtype is None else dtype, [gout, gin, w], _dwg_shapes(gin, gout, w, K) + [stride, pad, int(accum)])


def dwg_bwd_w(x, gout, dw, K, stride, pad, dtype=None):
    _call('dwg_bwd_w', _dt(x) if dtype is None else dtype, [x, gout, dw], _dwg_shapes(x, gout, dw, K) + [stride, pad])


def _bnx(op, dt, main, hw, act, y, scale, shift, dscale, other, out):
    npix, Cn = main.shape
    assert hw >= 1 and npix % hw == 0
    for n, t in (('y', y), ('post / g', other)):
        _need(t, npix * Cn, main.dtype, n, optional=True)
    _need(out, npix * Cn, main.dtype, 'out')
    _f32(scale, Cn, 'scale', optional=True)
    _f32(shift, Cn, 'shift', optional=True)
    _f32(dscale, npix // hw, 'dscale', optional=True)
    _call(op, dt, [y, scale, shift, dscale, other, out], [npix, hw, Cn, act])


def bnx_fwd(y, out, hw, act, scale=None, shift=None, dscale=None, post=None):
    _bnx('bnx_fwd', _dt(y), y, hw, act, y, scale, shift, dscale, post, out)


def bnx_bwd(g, out, hw, act, y=None, scale=None, shift=None, dscale=None, dtype=None):
    _bnx('bnx_bwd', _dt(g) if dtype is None else dtype, g, hw, act, y, scale, shift, dscale, g, out)


def dice_bwd(logits, target, sums, dlogits, loss_kind=0, grad_scale=1.0, dtype=None):
    """logits, target: f32 [B, C, HW]; sums: float64 [1 + B, C, 4] (totals first: I, S, T, BCE sum); dlogits: T [B, HW, CP]."""
    B, Cn, HW = logits.shape
    _f32(logits, B * Cn * HW, 'logits')
    _f32(target, B * Cn * HW, 'target')
    _need(sums, (1 + B) * Cn * 4, torch.float64, 'sums')
    assert dlogits.dim() == 3 and tuple(dlogits.shape[:2]) == (B, HW) and dlogits.shape[2] >= Cn
    _call('dice_bwd', _dt(dlogits) if dtype is None else dtype, [logits, target, sums, dlogits], [B, Cn, HW, dlogits.shape[2], loss_kind], [grad_scale])


# ---------------- GroupNorm + ReLU (+ bilinear x2), the squeeze-excite excitation
def gn_num_slabs(HW):
    return min(max(HW // 1024, 1), 64)


def gn_forward(y, gamma, beta, out, part, ss, stat, G, up, eps):
    N, H, W, Cn = y.shape
    _need(out, N * H * up * W * up * Cn, y.dtype, 'out')
    _f32(gamma, Cn, 'gamma')
    _f32(beta, Cn, 'beta')
    _f32(part, N * gn_num_slabs(H * W) * Cn * 2, 'part')
    _f32(ss, N * Cn * 2, 'ss')
    _f32(stat, N * G * 2, 'stat')
    _call('gn_forward', _dt(y), [y, gamma, beta, out, part, ss, stat], [N, H, W, Cn, G, up], [eps])


def gn_backward(y, g, dy, gamma, dgamma, dbeta, part, ss, stat, coef, G, dtype=None):
    N, HW, Cn = y.shape
    _need(g, N * HW * Cn, y.dtype, 'g')
    _need(dy, N * HW * Cn, y.dtype, 'dy')
    for n, t in (('gamma', gamma), ('dgamma', dgamma), ('dbeta', dbeta)):
        _f32(t, Cn, n)
    _f32(part, N * gn_num_slabs(HW) * Cn * 2, 'part')
    _f32(ss, N * Cn * 2, 'ss')
    _f32(stat, N * G * 2, 'stat')
    _f32(coef, N * G * 2, 'coef')
    _call('gn_backward', _dt(y) if dtype is None else dtype, [y, g, dy, gamma, dgamma, dbeta, part, ss, stat, coef], [N, HW, Cn, G])


def sefc_fwd(m, s, w1, b1, w2, b2, h, act):
    N, Cn = m.shape
    Rn = w1.shape[0]
    _need(s, N * Cn, m.dtype, 's')
    _f32(w1, Rn * Cn, 'w1')
    _f32(b1, Rn, 'b1')
    _f32(w2, Cn * Rn, 'w2')
    _f32(b2, Cn, 'b2')
    _f32(h, N * Rn, 'h')
    _call('sefc_fwd', _dt(m), [m, s, w1, b1, w2, b2, h], [N, Cn, Rn, act])


def sefc_bwd(m, ds, dm, w1, w2, h, dh, act, dw1=None, db1=None, dw2=None, db2=None, dtype=None):
    N, Cn = m.shape
    Rn = w1.shape[0]
    _need(ds, N * Cn, m.dtype, 'ds')
    _need(dm, N * Cn, m.dtype, 'dm')
    _f32(w1, Rn * Cn, 'w1')
    _f32(w2, Cn * Rn, 'w2')
    _f32(h, N * Rn, 'h')
    _f32(dh, N * Rn, 'dh')
    _f32(dw1, Rn * Cn, 'dw1', optional=True)
    _f32(db1, Rn, 'db1', optional=True)
    _f32(dw2, Cn * Rn, 'dw2', optional=True)
    _f32(db2, Cn, 'db2', optional=True)
    _call('sefc_bwd', _dt(m) if dtype is None else dtype, [m, ds, dm, w1, w2, h, dh, dw1, db1, dw2, db2], [N, Cn, Rn, act])
