"""CPU side of the single-op sweep tests (tests/test_gpu_sweeps.py): keeps the references honest.

- each float64 reference of tests/sweep_ref.py against torch.nn.functional / autograd on NCHW float64;
- every Rule X input set evaluated in float32 and in float64: the two must agree, which proves the "exact" inputs exact before
  a GPU sees them;
- the tolerance helpers and the guarded buffers on hand-made cases;
- the refusals of octseg_sweep_op through the library's host side (every refusal happens before any launch, so no GPU is needed).
"""
import pytest
import torch
import torch.nn.functional as F

import sweep_cases as SC
import sweep_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import sweeps as S

D = torch.float64


def _close(a, b, tol=1e-12):
    assert a.shape == b.shape and float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


# ------------------------------------------------------------------------------------------------ references against torch
def test_batchnorm_references_match_torch_forward():
    g = R.gen(1)
    x = torch.randn(3, 5, 6, 7, generator=g, dtype=D)                  # NCHW
    gamma, beta = torch.randn(5, generator=g, dtype=D), torch.randn(5, generator=g, dtype=D)
    rm, rv = torch.randn(5, generator=g, dtype=D), torch.rand(5, generator=g, dtype=D) + 0.5
    y = R.to_nhwc(x).reshape(-1, 5)
    rm_t, rv_t = rm.clone(), rv.clone()
    want = F.batch_norm(x, rm_t, rv_t, gamma, beta, True, 0.1, 1e-5)
    st = R.bn_finalize_small(y, gamma, beta, rm, rv, 0.1, 1e-5)
    _close(st['running_mean'], rm_t)
    _close(st['running_var'], rv_t)
    out, _ = R.bn_act(y, st['scale'], st['shift'])
    _close(out, R.to_nhwc(want).reshape(-1, 5))
    # the slab form (sum, sum of squares in row partials) gives the same statistics
    slab = torch.stack([y.view(9, -1, 5).sum(1), (y * y).view(9, -1, 5).sum(1)], -1)
    st2 = R.bn_finalize_train(slab, y.shape[0], gamma, beta, rm, rv, 0.1, 1e-5)
    for k in st:
        _close(st2[k], st[k], 1e-10)
    # eval / frozen: the running statistics
    ev = R.bn_finalize_eval(gamma, beta, rm, rv, 1e-5)
    out, _ = R.bn_act(y, ev['scale'], ev['shift'], relu=True)
    _close(out, R.to_nhwc(F.relu(F.batch_norm(x, rm, rv, gamma, beta, False, 0.0, 1e-5))).reshape(-1, 5))
    # residual forms: relu(bn(y) + bn'(res)) + post
    res, post = torch.randn_like(y), torch.randn_like(y)
    out, mag = R.bn_act(y, st['scale'], st['shift'], res, ev['scale'], ev['shift'], post, relu=True)
    _close(out, F.relu(y * st['scale'] + st['shift'] + res * ev['scale'] + ev['shift']) + post)
    assert bool((mag >= out.abs() - 1e-12).all())


@pytest.mark.parametrize('relu', [False, True])
def test_batchnorm_backward_references_match_autograd(relu):
    g = R.gen(2)
    npix, Cn, eps = 77, 6, 1e-5
    y, gr = torch.randn(npix, Cn, generator=g, dtype=D), torch.randn(npix, Cn, generator=g, dtype=D)
    gamma, beta = torch.randn(Cn, generator=g, dtype=D), torch.randn(Cn, generator=g, dtype=D)
    st = R.bn_finalize_small(y, gamma, beta, torch.zeros(Cn, dtype=D), torch.ones(Cn, dtype=D), 0.1, eps)
    dz = gr
    if relu:      # mask 1 recomputes the sign from y; mask 2 reads it from the output or from bn_act's bits: the same set
        out, _ = R.bn_act(y, st['scale'], st['shift'], relu=True)
        dz = R.bn_bwd_mask(gr, y, 2, out=out)
        assert torch.equal(dz, R.bn_bwd_mask(gr, y, 2, maskpos=out > 0))
        assert torch.equal(dz, R.bn_bwd_mask(gr, y, 1, st['scale'], st['shift']))
    rows, tpv = 5, 4
    slab, sa, n = R.bn_bwd_reduce(dz, y, st['mean'], st['rstd'], rows, tpv)
    assert float(n.sum()) == npix and bool((sa >= slab.abs() - 1e-12).all())
    s = slab.sum(0)
    dy, mag = R.bn_bwd_apply(dz, y, st['mean'], st['rstd'], gamma, s / npix)
    dx, dgamma, dbeta = R.bn_backward_autograd(y, gr, gamma, beta, eps, relu)
    _close(dy, dx, 1e-10)
    _close(s[:, 1], dgamma, 1e-10)
    _close(s[:, 0], dbeta, 1e-10)
    assert bool((mag >= dy.abs() - 1e-12).all())


def test_pool_and_plumbing_references_match_torch():
    g = R.gen(3)
    x = torch.randint(-6, 7, (2, 6, 10, 5), generator=g).to(D) * 0.5      # NHWC, multiples of 0.5: ties abound
    x[0, :2, :2] = float('-inf')
    out, idx = R.maxpool_fwd(x)
    want, widx = F.max_pool2d(R.to_nchw(x), 3, 2, 1, return_indices=True)
    assert torch.equal(out, R.to_nhwc(want))
    # window position -> flat input index, as torch reports it (the first maximum in scan order); windows of -inf only keep 255
    N, OH, OW, Cn = out.shape
    oy, ox = torch.arange(OH).view(1, OH, 1, 1), torch.arange(OW).view(1, 1, OW, 1)
    flat = (2 * oy - 1 + idx.long() // 3) * 10 + (2 * ox - 1 + idx.long() % 3)
    live = idx != 255
    assert torch.equal(flat[live], R.to_nhwc(widx)[live]) and bool((out[~live] == float('-inf')).all()) and int((~live).sum()) == 5
    # backward from the indices == autograd of max_pool2d (finite inputs)
    xf = torch.randint(-6, 7, (2, 6, 10, 5), generator=g).to(D) * 0.5
    gout = torch.randn(2, 3, 5, 5, generator=g, dtype=D)
    _, idx = R.maxpool_fwd(xf)
    xn = R.to_nchw(xf).clone().requires_grad_(True)
    (F.max_pool2d(xn, 3, 2, 1) * R.to_nchw(gout)).sum().backward()
    assert torch.equal(R.maxpool_bwd(idx, gout, 6, 10), R.to_nhwc(xn.grad))
    # nearest x2 and its adjoint
    a = torch.randn(2, 3, 5, 4, generator=g, dtype=D)
    assert torch.equal(R.up2(a), R.to_nhwc(F.interpolate(R.to_nchw(a), scale_factor=2, mode='nearest')))
    assert torch.equal(R.up2(a), R.to_nhwc(torch.nn.Upsample(scale_factor=2, mode='nearest')(R.to_nchw(a))))
    b = torch.randn(2, 6, 10, 4, generator=g, dtype=D)
    an = R.to_nchw(a).clone().requires_grad_(True)
    (F.interpolate(an, scale_factor=2, mode='nearest') * R.to_nchw(b)).sum().backward()
    _close(R.pool2x2(b), R.to_nhwc(an.grad))


@pytest.mark.parametrize('sizes', SC.RESIZES + (((3, 5), (5, 9)), ((260, 4), (260, 4))))
def test_bilinear_references_match_torch(sizes):
    """The references use the float32 source index torch's own float kernels use; against float64 interpolate they may differ by the
    rounding of the weights: at most 2 ulp of the coordinate (<= in - 1) per axis."""
    (IH, IW), (OH, OW) = sizes
    g = R.gen(4)
    x = torch.randn(2, IH, IW, 3, generator=g, dtype=D)
    ref, mag = R.bilinear_resize(x, OH, OW)
    want = R.to_nhwc(F.interpolate(R.to_nchw(x), size=(OH, OW), mode='bilinear', align_corners=True))
    tol = 4 * (max(IH, IW) + 1) * 2.0 ** -23
    assert bool(((ref - want).abs() <= tol * mag + 1e-15).all())
    f32 = R.to_nhwc(F.interpolate(R.to_nchw(x).float(), size=(OH, OW), mode='bilinear', align_corners=True)).double()      # torch's float kernel: the same weights
    assert bool(((ref - f32).abs() <= R.BILINEAR_K * R.EPS32 * mag).all())
    R.LERP_FUSED[0] = True      # the fused evaluation of the weights: within half an ulp of the coordinate of the other
    try:
        fused, _ = R.bilinear_resize(x, OH, OW)
    finally:
        R.LERP_FUSED[0] = False
    assert float((fused - ref).abs().max()) <= 2 * (IH + IW) * R.EPS32 * 4 * float(x.abs().max())
    go = torch.randn(2, OH, OW, 3, generator=g, dtype=D)
    xn = R.to_nchw(x).clone().requires_grad_(True)
    (F.interpolate(xn, size=(OH, OW), mode='bilinear', align_corners=True) * R.to_nchw(go)).sum().backward()
    adj, sa, nt = R.bilinear_adjoint(go, IH, IW)
    assert bool(((adj - R.to_nhwc(xn.grad)).abs() <= tol * sa + 1e-15).all())
    assert float(nt.max()) <= OH * OW and float(nt.min()) >= 1
    # <resize(x), go> == <x, adjoint(go)>
    assert abs(float((ref * go).sum() - (x * adj).sum())) <= 1e-9 * float((ref * go).abs().sum())


@pytest.mark.parametrize('k', [1, 2, 3, 6])
def test_bin_mean_references_match_torch(k):
    g = R.gen(5)
    for H, W in ((22, 22), (3, 5)):
        x = torch.randn(2, H, W, 4, generator=g, dtype=D)
        ref, sa, cnt = R.bin_mean(x, k)
        _close(ref, R.to_nhwc(F.adaptive_avg_pool2d(R.to_nchw(x), (k, k))))
        go = torch.randn(2, k, k, 4, generator=g, dtype=D)
        xn = R.to_nchw(x).clone().requires_grad_(True)
        (F.adaptive_avg_pool2d(xn, (k, k)) * R.to_nchw(go)).sum().backward()
        gin, _, nt = R.bin_mean_bwd(go, H, W)
        assert bool(((gin - R.to_nhwc(xn.grad)).abs() <= 4 * R.EPS32 * R.bin_mean_bwd(go.abs(), H, W)[0] + 1e-15).all())      # (1 / area is a float32)
        assert float(nt.min()) >= 1
    _close(R.bin_mean(x, 1)[0][:, 0, 0], x.mean((1, 2)))      # AdaptiveAvgPool2d(1) = image_sum / HW


def test_gate_and_rearrangement_references():
    g = R.gen(6)
    x, s, s2 = torch.randn(2, 9, 8, generator=g, dtype=D), torch.randn(2, 8, generator=g, dtype=D) * 3, torch.randn(2, 8, generator=g, dtype=D)
    _close(R.sigmoid_as_kernel(s), torch.sigmoid(s))
    out, _ = R.se_gate(x, s, None, s2)
    _close(out, x * (torch.sigmoid(s) + torch.sigmoid(s2)).unsqueeze(1))
    sv = s.clone().requires_grad_(True)
    gr = torch.randn(2, 9, 8, generator=g, dtype=D)
    (x * torch.sigmoid(sv).unsqueeze(1) * gr).sum().backward()
    _close(R.se_dgate(gr, x, s)[0], sv.grad)
    f = torch.randn(2, 6, 10, 3, generator=g, dtype=D)
    c = R.parity_to_coarse(f)
    assert c.shape == (8, 3, 5, 3) and torch.equal(c[4 * 1 + 2 * 1 + 0], f[1, 1::2, 0::2]) and torch.equal(R.parity_to_fine(c), f)
    for r in (2, 3):
        fm = torch.randn(2, 7, 5, 3, generator=g, dtype=D)
        m = R.to_mosaic(fm, r)
        assert torch.equal(R.from_mosaic(m, 7, 5, r), fm) and int((m != 0).sum()) == fm.numel()
        hs = -(-7 // r)
        assert torch.equal(m[:, 1 + 1 * (hs + 1) + 1, 1], fm[:, 1 * r + 1, 0]) and bool((m[:, 0] == 0).all()) and bool((m[:, :, 0] == 0).all())
        # a 3x3 / pad 1 conv on the mosaic == the dilation-r conv on the fine map
        w = torch.randn(3, 3, 3, 3, generator=g, dtype=D)
        conv_m = R.from_mosaic(R.to_nhwc(F.conv2d(R.to_nchw(m), w, padding=1)), 7, 5, r)
        _close(conv_m, R.to_nhwc(F.conv2d(R.to_nchw(fm), w, padding=r, dilation=r)))


@pytest.mark.parametrize('dil', [1, 2, 12])
def test_depthwise_references_match_grouped_conv2d(dil):
    g = R.gen(7)
    x, w = torch.randn(2, 8, 8, 5, generator=g, dtype=D), torch.randn(9, 5, generator=g, dtype=D)
    wt = w.t().reshape(5, 1, 3, 3).clone().requires_grad_(True)                 # [C, 1, r, s] <- w[3 r + s][c]
    xn = R.to_nchw(x).clone().requires_grad_(True)
    out = F.conv2d(xn, wt, padding=dil, dilation=dil, groups=5)
    ref, sa = R.dw_conv(x, w, dil)
    _close(ref, R.to_nhwc(out.detach()))
    assert bool((sa >= ref.abs() - 1e-12).all())
    go = torch.randn(2, 8, 8, 5, generator=g, dtype=D)
    (out * R.to_nchw(go)).sum().backward()
    _close(R.dw_conv(go, w, dil, flip=True)[0], R.to_nhwc(xn.grad))              # the data gradient: the mirrored kernel
    _close(R.dw_wgrad(x, go, dil)[0], wt.grad.reshape(5, 9).t())
    if dil == 12:      # only the centre tap is live on an 8 x 8 map
        _close(ref, x * w[4])


@pytest.mark.parametrize('K,stride,H', [(3, 1, 8), (3, 2, 8), (3, 2, 7), (5, 2, 8), (5, 2, 9), (5, 1, 7)])
def test_strided_depthwise_references_match_grouped_conv2d(K, stride, H):
    """TF static "same" padding: total (OH - 1) stride + K - H, the smaller half on top / left (an F.pad in front of conv2d)."""
    g = R.gen(8)
    W = H
    OH, pad = R.tf_same(H, K, stride)
    tot = max((OH - 1) * stride + K - H, 0)
    x, w = torch.randn(2, H, W, 5, generator=g, dtype=D), torch.randn(K, K, 5, generator=g, dtype=D)
    wt = w.permute(2, 0, 1).unsqueeze(1).clone().requires_grad_(True)
    xn = R.to_nchw(x).clone().requires_grad_(True)
    out = F.conv2d(F.pad(xn, (pad, tot - pad, pad, tot - pad)), wt, stride=stride, groups=5)
    assert out.shape[2] == OH
    ref, sa = R.dwg_fwd(x, w, OH, OH, K, stride, pad)
    _close(ref, R.to_nhwc(out.detach()))
    go = torch.randn(2, OH, OH, 5, generator=g, dtype=D)
    (out * R.to_nchw(go)).sum().backward()
    gin, _, nt = R.dwg_bwd_data(go, w, H, W, K, stride, pad)
    _close(gin, R.to_nhwc(xn.grad))
    _close(R.dwg_bwd_w(x, go, K, stride, pad)[0], wt.grad.squeeze(1).permute(1, 2, 0))
    assert float(nt.max()) <= K * K


def test_groupnorm_swish_fc_and_dice_references_match_torch():
    g = R.gen(9)
    N, H, W, Cn, G = 2, 4, 6, 16, 4
    y = torch.randn(N, H * W, Cn, generator=g, dtype=D)
    gamma, beta, gr = torch.randn(Cn, generator=g, dtype=D), torch.randn(Cn, generator=g, dtype=D), torch.randn(N, H * W, Cn, generator=g, dtype=D)
    ss, stat = R.gn_stats(y, gamma, beta, G, 1e-5)
    yn = R.to_nchw(y.view(N, H, W, Cn)).clone().requires_grad_(True)
    gam, bet = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    act = F.relu(F.group_norm(yn, G, gam, bet, 1e-5))
    _close(R.gn_act(y, ss, H, W, 1)[0], R.to_nhwc(act.detach()), 1e-10)
    up = F.interpolate(act, scale_factor=2, mode='bilinear', align_corners=True)
    assert float((R.gn_act(y, ss, H, W, 2)[0] - R.to_nhwc(up.detach())).abs().max()) < 1e-5      # (float32 weights)
    (act * R.to_nchw(gr.view(N, H, W, Cn))).sum().backward()
    r = R.gn_backward(y, gr, gamma, ss, stat, G)
    _close(r['dy'], R.to_nhwc(yn.grad).reshape(N, H * W, Cn), 1e-9)
    _close(r['dgamma'], gam.grad, 1e-9)
    _close(r['dbeta'], bet.grad, 1e-9)
    # BatchNorm + swish sweep and its gradient
    z0 = torch.randn(6, 8, generator=g, dtype=D).requires_grad_(True)
    sc, sh, dsc, post = torch.randn(8, generator=g, dtype=D), torch.randn(8, generator=g, dtype=D), torch.rand(2, generator=g, dtype=D), torch.randn(6, 8, generator=g, dtype=D)
    zz = z0 * sc + sh
    o = F.silu(zz) * dsc.repeat_interleave(3).unsqueeze(1) + post
    _close(R.bnx_fwd(z0, 3, 1, sc, sh, dsc, post)[0], o.detach(), 1e-12)
    g2 = torch.randn(6, 8, generator=g, dtype=D)
    gz, = torch.autograd.grad((o * g2).sum(), zz)
    _close(R.bnx_bwd(g2, 3, 1, z0, sc, sh, dsc)[0], gz, 1e-12)
    # the two FCs of the squeeze-excite, both activations
    for a in (0, 1):
        m = torch.randn(3, 10, generator=g, dtype=D).requires_grad_(True)
        w1, b1 = torch.randn(4, 10, generator=g, dtype=D).requires_grad_(True), torch.randn(4, generator=g, dtype=D).requires_grad_(True)
        w2, b2 = torch.randn(10, 4, generator=g, dtype=D).requires_grad_(True), torch.randn(10, generator=g, dtype=D).requires_grad_(True)
        hh = F.linear(m, w1, b1)
        s_ = F.linear(F.silu(hh) if a else F.relu(hh), w2, b2)
        s_ref, h_ref, _ = R.sefc_fwd(m, w1, b1, w2, b2, a)
        _close(s_ref, s_.detach(), 1e-12)
        ds = torch.randn(3, 10, generator=g, dtype=D)
        (s_ * ds).sum().backward()
        rb = R.sefc_bwd(m, ds, w1, w2, h_ref, a)
        for k, t in (('dm', m), ('dw1', w1), ('db1', b1), ('dw2', w2), ('db2', b2)):
            _close(rb[k], t.grad, 1e-10)
    # Dice (multilabel, from logits) and mean BCE: autograd of the losses
    B, C_, HW = 2, 3, 50
    z = (torch.randn(B, C_, HW, generator=g) * 2).requires_grad_(True)
    t = (torch.rand(B, C_, HW, generator=g) < 0.3).float()
    t[:, 2] = 0
    sums = R.dice_sums(z, t)
    zd = z.double()
    p = torch.sigmoid(zd)
    I_, S_ = (p * t).sum((0, 2)), (p + t).sum((0, 2))
    dice = ((1 - 2 * I_ / S_.clamp_min(1e-7)) * (t.sum((0, 2)) > 0)).mean()
    bce = F.binary_cross_entropy_with_logits(zd, t.double())
    for kind, loss in ((0, dice), (1, bce), (2, dice + bce)):
        gz, = torch.autograd.grad(loss * 0.5, z, retain_graph=True)
        ref, mag = R.dice_bwd(z, t, sums, kind, 0.5)
        assert float((ref - gz.double().permute(0, 2, 1)).abs().max()) < 2e-7 * max(1.0, float(gz.abs().max())) + 1e-9      # (the totals pass through float)
        assert bool((mag >= ref.abs() - 1e-12).all())


# ------------------------------------------------------------------------------------------------ Rule X inputs are exact
@pytest.mark.parametrize('family', sorted(SC.FAMILIES))
def test_rule_x_input_sets_are_exact(family):
    """Evaluated in float32 and in float64 the references agree, and what is stored as T is a float32 already."""
    seen = 0
    for case in SC.FAMILIES[family]():
        if case.refs is None:
            continue
        big = getattr(case, 'big', False)
        refs = case.sample_refs if big else case.refs      # the 84 M-element case: a strided sample of its pixels
        r64 = refs()
        with R.as_float32():
            r32 = refs()
        assert set(r64) == set(r32) and r64
        for k in r64:
            assert torch.equal(r32[k].to(r64[k].dtype), r64[k]), f'{case.id}: {k} differs between float32 and float64'
            shape = case.outs[k][0] if k in case.outs else tuple(case.ins[k].shape)      # (an input name: the output aliases it)
            assert big or r64[k].numel() == torch.Size(shape).numel(), f'{case.id}: {k}'
            if r64[k].dtype.is_floating_point:
                assert R.is_f32_exact(r64[k]), f'{case.id}: {k} is not a float32'
        seen += 1
    assert seen > 0 or family == 'dice_bwd'      # (its exact part is the zero padding; the values are transcendental)


def test_every_family_has_exact_cases_and_every_trainonly_op_is_listed():
    n_exact = {f: sum(c.refs is not None for c in fn()) for f, fn in SC.FAMILIES.items()}
    assert all(n > 0 for f, n in n_exact.items() if f != 'dice_bwd'), n_exact
    assert {t[0] for t in SC.TRAIN_ONLY} <= set(S.OP_NAMES)


# ------------------------------------------------------------------------------------------------ the helpers themselves
def test_tolerance_helpers_on_hand_made_cases():
    one = torch.tensor([1.0], dtype=D)
    # Rule X: one ulp off fails, the once-rounded value passes; bf16 rounds 1 + 2^-8 (a tie) to even
    R.assert_exact(torch.tensor([1.0], dtype=torch.bfloat16), one + 2.0 ** -8)
    R.assert_exact(torch.tensor([1.0 + 2.0 ** -6], dtype=torch.bfloat16), one + 3 * 2.0 ** -8)
    with pytest.raises(AssertionError):
        R.assert_exact(torch.tensor([1.0 + 2.0 ** -7], dtype=torch.bfloat16), one)
    with pytest.raises(AssertionError):
        R.assert_exact(torch.tensor([1.0 + 2.0 ** -23]), one)
    with pytest.raises(AssertionError):
        R.assert_exact(torch.tensor([float('nan')]), one)
    with pytest.raises(AssertionError):      # not a float32: a double rounding would hide behind the conversion
        R.assert_exact(torch.tensor([1.0], dtype=torch.float16), one + 2.0 ** -30)
    R.assert_exact(torch.tensor([3, 255], dtype=torch.uint8), torch.tensor([3, 255], dtype=torch.uint8))
    with pytest.raises(AssertionError):
        R.assert_exact(torch.tensor([3, 254], dtype=torch.uint8), torch.tensor([3, 255], dtype=torch.uint8))
    # Rule E: u_T |ref| + k eps32 mag
    b = R.bound_e(one, 3 * one, 4, torch.bfloat16)
    assert float(b) == 2.0 ** -8 + 12 * 2.0 ** -24
    assert float(R.bound_e(one, 3 * one, 4, torch.float32)) == 13 * 2.0 ** -24
    assert float(R.bound_e(one * 2.0 ** -20, 0 * one, 0, torch.float16)) == 2.0 ** -25 and float(R.bound_e(one * 2.0 ** -13, 0 * one, 0, torch.float16)) == 2.0 ** -24
    R.assert_within(torch.tensor([1.0 + 2.0 ** -8], dtype=D), one, b)
    with pytest.raises(AssertionError):
        R.assert_within(torch.tensor([1.0 + 2.0 ** -7], dtype=D), one, b)
    with pytest.raises(AssertionError):      # a NaN never passes
        R.assert_within(torch.tensor([float('nan')], dtype=D), one, b)
    # Rule R: n eps32 sum|terms| (+ u_T |ref|)
    assert float(R.bound_r(one, 10 * one, 100)) == 1000 * 2.0 ** -24
    assert float(R.bound_r(one, 10 * one, 100, torch.float16)) == 1000 * 2.0 ** -24 + 2.0 ** -11
    # Rule T: 4 x the yardstick's largest distance, never below the Rule E bound
    ref = torch.tensor([1.0, 2.0], dtype=D)
    yard = torch.tensor([1.0 + 1e-6, 2.0], dtype=D)
    n0 = len(R.RATIOS)
    R.assert_transcendental(torch.tensor([1.0, 2.0 + 3.9e-6], dtype=D), ref, yard, torch.zeros(2, dtype=D), 'hand', torch.float32)
    assert R.RATIOS[-1][0] == 'hand' and abs(R.RATIOS[-1][2] - 3.9) < 1e-3
    with pytest.raises(AssertionError):
        R.assert_transcendental(torch.tensor([1.0, 2.0 + 4.1e-6], dtype=D), ref, yard, torch.zeros(2, dtype=D), 'hand', torch.float32)
    R.assert_transcendental(torch.tensor([1.0, 2.0 + 4.1e-6], dtype=D), ref, yard, torch.full((2,), 5e-6, dtype=D), 'hand', torch.float32)
    del R.RATIOS[n0:]
    # mask bits
    pos = torch.tensor([[True, False, False, True, False, False, False, True]])
    assert R.pack_mask(pos, 8).tolist() == [[1 + 8 + 128]] and R.pack_mask(pos, 4).tolist() == [[9, 8]]
    assert torch.equal(SC._unpack_mask(R.pack_mask(pos, 4), 4), pos)


def test_guarded_buffers_catch_writes_outside():
    G = R.Guard(torch.device('cpu'))
    a = G.put(torch.arange(6, dtype=torch.float32).view(2, 3))
    b = G.empty((5,), torch.bfloat16)
    m = G.empty((3,), torch.uint8)
    assert a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0 and bool(torch.isnan(b.float()).all()) and m.tolist() == [255] * 3
    assert a.tolist() == [[0, 1, 2], [3, 4, 5]] and len(G.bufs) == 3 and G.bufs[0][0].numel() == 2 * R.MARGIN + 32
    G.check()
    buf, nbytes = G.bufs[1]
    assert bool(torch.isnan(buf[:R.MARGIN].view(torch.float32)).all())      # the margins read as NaN
    buf[R.MARGIN + nbytes] = 0       # the first byte behind the interior (inside the 16-byte padding)
    with pytest.raises(AssertionError):
        G.check()
    buf[R.MARGIN + nbytes] = R.FILL
    G.bufs[0][0][R.MARGIN - 1] = 7   # the last byte in front of a buffer
    with pytest.raises(AssertionError):
        G.check()


# ------------------------------------------------------------------------------------------------ refusals (host side, no launch)
A = 0x10000      # an aligned address that is never dereferenced: every call below is refused before any launch


def _rc(op, dtype, nptrs, iargs, fargs=(), ptrs=None):
    return S.sweep_op_raw(op, dtype, [A] * nptrs if ptrs is None else ptrs, iargs, fargs)


def test_sweep_op_refusals():
    lib = L.lib()
    OK, BAD_SHAPE, BAD_DTYPE, BAD_ARG = 0, -1, -2, -5
    assert len(S.OP_NAMES) == len(set(S.OP_NAMES))
    assert _rc(len(S.OP_NAMES), L.F32, 2, (1,)) == BAD_ARG and _rc(-1, L.F32, 2, (1,)) == BAD_ARG      # unknown op
    assert b'unknown op' in lib.octseg_last_error()
    assert _rc('add2', 7, 3, (8,)) == BAD_DTYPE
    for op, nptrs, ia, fa in SC.TRAIN_ONLY:      # f16 on a training-only sweep
        assert _rc(op, L.F16, nptrs, ia, fa) == BAD_DTYPE, op
        assert b'f16' in lib.octseg_last_error()
    # counts that do not match the op
    assert _rc('add2', L.F32, 2, (8,)) == BAD_ARG and _rc('add2', L.F32, 3, (8, 1)) == BAD_ARG and _rc('add2', L.F32, 3, (8,), (1.0,)) == BAD_ARG
    # null required pointers; optional ones may be null (checked on a call that is then refused for its shape)
    assert _rc('add2', L.F32, 3, (8,), ptrs=[A, None, A]) == BAD_ARG and b'null' in lib.octseg_last_error()
    assert _rc('relu', L.F32, 3, (7,), ptrs=[A, None, A]) == BAD_SHAPE
    assert _rc('bn_act', L.BF16, 9, (4, 8, 1), ptrs=[A, A, None, None, None, None, None, A, None]) == BAD_ARG       # scale without shift
    assert _rc('bn_act', L.BF16, 9, (4, 8, 1), ptrs=[A, None, None, None, A, A, None, A, None]) == BAD_ARG          # rscale without res
    assert _rc('bn_act', L.BF16, 9, (4, 8, 1), ptrs=[None, None, None, None, None, None, None, A, None]) == BAD_ARG
    bw = [A] * 17
    bw[2] = bw[3] = None
    assert _rc('bn_bwd_apply', L.F32, 17, (4, 8, 2, 1, 0), ptrs=bw) == BAD_ARG and b'mask 2' in lib.octseg_last_error()
    assert _rc('bn_bwd_apply', L.F32, 17, (4, 8, 3, 1, 0)) == BAD_ARG
    assert _rc('se_dgate', L.F32, 7, (1, 4, 8), ptrs=[A, A, A, A, A, A, None]) == BAD_ARG
    # misaligned pointers
    assert _rc('add2', L.F32, 3, (8,), ptrs=[A, A + 4, A]) == BAD_ARG and b'aligned' in lib.octseg_last_error()
    assert _rc('channel_sum', L.F32, 2, (4, 8, 3), ptrs=[A + 8, A]) == BAD_ARG
    # C % VEC, empty tensors
    assert _rc('bn_act', L.F32, 9, (4, 6, 1)) == BAD_SHAPE and _rc('bn_act', L.BF16, 9, (4, 12, 1)) == BAD_SHAPE and _rc('bn_act', L.F16, 9, (4, 4, 1)) == BAD_SHAPE
    assert _rc('bn_act', L.F32, 9, (0, 8, 1)) == BAD_SHAPE and _rc('bn_act', L.F32, 9, (-4, 8, 1)) == BAD_SHAPE and _rc('bn_act', L.F32, 9, (2 ** 31, 8, 1)) == BAD_SHAPE
    for op, nptrs, ia in (('bn_bwd_reduce', 17, (4, 12, 0, 1, 0)), ('tensor_stats', 2, (4, 12, 1)), ('pool2x2_accum', 2, (1, 2, 2, 12, 1)),
                          ('up2_fill', 2, (1, 2, 2, 12)), ('maxpool_fwd', 3, (1, 2, 2, 12)), ('bilinear_resize', 2, (1, 2, 2, 4, 4, 12)),
                          ('bin_mean', 2, (1, 4, 4, 12, 2)), ('parity_permute', 2, (1, 2, 2, 12, 1, 0)), ('mosaic', 2, (1, 4, 4, 12, 2, 1, 0))):
        assert _rc(op, L.BF16, nptrs, ia) == BAD_SHAPE, op
    assert _rc('masked_accum', L.BF16, 3, (12, 1)) == BAD_SHAPE and _rc('drop_elem', L.F32, 3, (6,), (1.0,)) == BAD_SHAPE
    for op, nptrs, ia, fa in (('image_sum', 2, (1, 4, 12), (4.0,)), ('image_bcast', 2, (1, 4, 12, 0), (1.0,)), ('se_gate', 4, (1, 4, 12, 0), ()),
                              ('merge_drop', 6, (1, 4, 12), (1.0,)), ('drop_bwd', 3, (1, 4, 12), (1.0,))):
        assert _rc(op, L.BF16, nptrs, ia, fa) == BAD_SHAPE, op
    # odd H or W for the 2x pools and the parity permute; k < 1; rows < 1; up < 2; count beyond the small path
    assert _rc('maxpool_fwd', L.F32, 3, (1, 3, 4, 8)) == BAD_SHAPE and _rc('maxpool_bwd_idx', L.F32, 3, (1, 4, 5, 8, 1)) == BAD_SHAPE
    assert _rc('parity_permute', L.F32, 2, (1, 4, 5, 8, 1, 0)) == BAD_SHAPE
    assert _rc('bin_mean', L.F32, 2, (1, 4, 4, 8, 0)) == BAD_SHAPE and _rc('bin_mean_bwd', L.F32, 2, (1, 4, 4, 8, 0, 0)) == BAD_SHAPE
    assert _rc('mosaic', L.F32, 2, (1, 4, 4, 8, 0, 1, 0)) == BAD_SHAPE
    assert _rc('tensor_stats', L.F32, 2, (4, 8, 0)) == BAD_SHAPE and _rc('bn_bwd_reduce', L.F32, 17, (4, 8, 0, 0, 0)) == BAD_SHAPE
    assert _rc('bn_finalize_train', L.F32, 11, (0, 8), (4.0, 0.1, 1e-5)) == BAD_SHAPE and _rc('bn_finalize_train', L.F32, 11, (1, 8), (0.0, 0.1, 1e-5)) == BAD_SHAPE
    assert _rc('bilinear_adjoint', L.F32, 2, (1, 2, 2, 8, 1)) == BAD_SHAPE
    assert _rc('bn_finalize_small', L.F32, 9, (1025, 8), (0.1, 1e-5)) == BAD_SHAPE and _rc('bn_bwd_small', L.F32, 17, (1025, 8, 0, 1, 0)) == BAD_SHAPE
    assert _rc('channel_sum', L.F32, 2, (4, 2, 3)) == BAD_SHAPE       # C > Cstride
    assert _rc('bilinear_resize_adjoint', L.F32, 2, (1, 65537, 65537, 4, 4, 4)) == BAD_SHAPE
    # depthwise slices: outside the tensor, off a vector boundary, dilation 0; the CAM seed's padded width
    ok = [24, 8, 16, 8, 16, 4, 1, 4, 4, 8, 1, 0, 0]      # inC, ic0, outC, oc0, wC, wc0, N, H, W, C, dil, flip, accum
    for i, v in ((1, 24), (3, 16), (5, 12), (1, 4), (4, 14), (5, 2), (10, 0), (9, 12)):
        bad = list(ok)
        bad[i] = v
        assert _rc('dw_conv', L.BF16, 3, bad) == BAD_SHAPE, (i, v)
        assert _rc('dw_wgrad', L.BF16, 3, bad[:11]) == BAD_SHAPE, (i, v)
    assert _rc('cam_seed', L.BF16, 2, (1, 3, 4, 12)) == BAD_SHAPE and _rc('cam_seed', L.BF16, 2, (1, 9, 4, 8)) == BAD_SHAPE
    assert _rc('cam_seed', L.F32, 2, (1, 3, 0, 8)) == BAD_SHAPE and _rc('cam_seed', L.F32, 2, (1, 3, 4, 24)) == BAD_SHAPE
    # GroupNorm widths whose vector count does not divide 256, groups that do not divide C, up = 4
    for Cn, G_ in ((24, 3), (48, 6), (304, 19), (2048, 32), (128, 5)):
        assert _rc('gn_forward', L.BF16, 7, (1, 4, 4, Cn, G_, 1), (1e-5,)) == BAD_SHAPE, Cn
        assert _rc('gn_backward', L.BF16, 10, (1, 16, Cn, G_)) == BAD_SHAPE, Cn
    assert b'256' in lib.octseg_last_error() or b'group' in lib.octseg_last_error()
    assert _rc('gn_forward', L.F32, 7, (1, 4, 4, 128, 32, 4), (1e-5,)) == BAD_SHAPE and _rc('gn_forward', L.F32, 7, (1, 4, 4, 2048, 32, 1), (1e-5,)) == BAD_SHAPE
    # strided depthwise: kernel size, stride, padding, an output map that does not fit
    okd = [1, 8, 8, 8, 4, 4, 3, 2, 0]      # N, H, W, C, OH, OW, K, stride, pad
    for i, v in ((6, 4), (6, 7), (7, 3), (7, 0), (8, 3), (4, 6), (5, 0), (3, 12)):
        bad = list(okd)
        bad[i] = v
        assert _rc('dwg_fwd', L.BF16, 3, bad) == BAD_SHAPE and _rc('dwg_bwd_w', L.BF16, 3, bad) == BAD_SHAPE and _rc('dwg_bwd_data', L.BF16, 3, bad + [0]) == BAD_SHAPE, (i, v)
    # BatchNorm + swish: act, scale without shift, the swish gradient without y, a pixel count that is no multiple of hw
    assert _rc('bnx_fwd', L.F32, 6, (8, 4, 8, 2)) == BAD_ARG and _rc('bnx_fwd', L.F32, 6, (8, 3, 8, 1)) == BAD_SHAPE and _rc('bnx_fwd', L.F32, 6, (8, 4, 6, 1)) == BAD_SHAPE
    assert _rc('bnx_fwd', L.F32, 6, (8, 4, 8, 1), ptrs=[A, A, None, None, None, A]) == BAD_ARG
    assert _rc('bnx_bwd', L.F32, 6, (8, 4, 8, 1), ptrs=[None, A, A, None, A, A]) == BAD_ARG and _rc('bnx_bwd', L.F32, 6, (8, 4, 8, 1), ptrs=[A, None, None, None, A, A]) == BAD_ARG
    assert _rc('dice_bwd', L.F32, 4, (1, 3, 4, 12, 0), (1.0,)) == BAD_SHAPE and _rc('dice_bwd', L.F32, 4, (1, 9, 4, 8, 0), (1.0,)) == BAD_SHAPE
    assert _rc('dice_bwd', L.F32, 4, (1, 3, 4, 8, 3), (1.0,)) == BAD_ARG
    assert _rc('sefc_fwd', L.F32, 7, (1, 8, 0, 1)) == BAD_SHAPE and _rc('sefc_fwd', L.F32, 7, (1, 16000, 8, 1)) == BAD_SHAPE and _rc('sefc_fwd', L.F32, 7, (1, 8, 2, 2)) == BAD_ARG
    assert _rc('sefc_bwd', L.F32, 11, (1, 8, 2, 1), ptrs=[A] * 8 + [None, A, A]) == BAD_ARG


def test_wrappers_check_buffer_extents_before_the_call():
    """The extents of every buffer follow from the shapes; a tensor of another size or dtype never reaches the library."""
    x = torch.zeros(4, 8)
    with pytest.raises(AssertionError):
        S.add2(x, torch.zeros(4, 7), torch.zeros(4, 8))
    with pytest.raises(AssertionError):
        S.bn_act(x, torch.zeros(4, 8), scale=torch.zeros(7), shift=torch.zeros(8))
    with pytest.raises(AssertionError):
        S.bn_act(x, torch.zeros(4, 8), maskbits=torch.zeros(4, 1, dtype=torch.uint8))       # f32: two vectors per pixel
    with pytest.raises(AssertionError):
        S.bn_bwd_reduce(x, x, *[torch.zeros(8)] * 4, torch.zeros(2, 8, 2, dtype=torch.float64))
    with pytest.raises(AssertionError):
        S.maxpool_fwd(torch.zeros(1, 4, 4, 8), torch.zeros(1, 2, 2, 8), torch.zeros(1, 2, 2, 4, dtype=torch.uint8))
    with pytest.raises(AssertionError):
        S.se_dgate(torch.zeros(1, 128, 8), torch.zeros(1, 128, 8), torch.zeros(1, 8), torch.zeros(1, 8), torch.zeros(1, 1, 8))      # two shares
    with pytest.raises(AssertionError):
        S.bn_finalize_train(torch.zeros(3, 8, 2), 4.0, *[torch.zeros(8)] * 4, 0.1, 1e-5, *[torch.zeros(8)] * 4, torch.zeros(100, dtype=torch.float64),
                            torch.zeros(64, dtype=torch.int32))
    assert S.se_dgate_shares(63) == 1 and S.se_dgate_shares(128) == 2 and S.se_dgate_shares(10 ** 6) == 64 and S.mosaic_extent(7, 5, 3) == (13, 10)
