"""CPU half of the single-stage tests of pan.hip's pyramid kernels and pab.hip's attention kernels (tests/test_gpu_blockops.py is the GPU half):

- the float64 references of tests/block_ref.py against torch.nn.functional / autograd in NCHW float64, and the restated pyramid / PAB
  against oracle/nets.py's FPABlock / PAB;
- every Rule X input set evaluated in float32 and in float64 (they must agree, and be float32 numbers);
- the kink margins of the pyramid seeds the GPU cases use;
- the scratch layouts of blockops.py against the library's own sizes, and the wrappers' extent checks;
- the refusals of octseg_fpa_op / octseg_pab_op through the library's host side (every refusal happens before any launch: no GPU needed).
"""
import pytest
import torch
import torch.nn.functional as F

import block_cases as BC
import block_ref as BR
import sweep_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import blockops as B
from oracle import nets

D = torch.float64


def close(a, b, tol=1e-11):
    a, b = a.to(D), b.to(D)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), float((a - b).abs().max())


def nchw(x):
    return x.permute(0, 3, 1, 2)


# ------------------------------------------------------------------------------------------------ references against torch
def test_maxpool2_references_match_torch_with_ties():
    g = R.gen(1)
    x = BC._maxpool_x((3, 6, 4, 8), torch.float32, g).to(D)
    dp = R.dyadic((3, 3, 2, 8), torch.float32, g).to(D)
    xt = nchw(x).clone().requires_grad_(True)
    out, idx = F.max_pool2d(xt, 2, 2, return_indices=True)
    assert torch.equal(BR.maxpool2_fwd(x), out.detach().permute(0, 2, 3, 1))
    # the first maximum in scan order: torch's flat index into the H x W plane
    am = BR.maxpool2_argmax(x)
    oy, ox = torch.arange(3).view(1, 3, 1, 1), torch.arange(2).view(1, 1, 2, 1)
    flat = (2 * oy + am // 2) * 4 + 2 * ox + am % 2
    assert torch.equal(flat, idx.permute(0, 2, 3, 1))
    assert int((BR._quads(x) == BR._quads(x).max(0).values).sum(0).max()) == 4      # a fully tied window exists
    out.backward(nchw(dp))
    assert torch.equal(BR.maxpool2_bwd(x, dp), xt.grad.permute(0, 2, 3, 1))
    dx0 = R.dyadic(x.shape, torch.float32, g)
    assert torch.equal(BR.maxpool2_bwd(x, dp, dx0), xt.grad.permute(0, 2, 3, 1) + dx0)
    # floor mode on an odd one-channel map (the pyramid's 11 -> 5)
    m = torch.randn(2, 11, 7, generator=g, dtype=D)
    assert torch.equal(BR.pyr_maxpool(m), F.max_pool2d(m.unsqueeze(1), 2, 2)[:, 0])


@pytest.mark.parametrize('shape', [(2, 4, 4, 8), (1, 2, 3, 12), (2, 11, 7, 5)])
def test_wide_conv_references_match_conv2d(shape):
    g = R.gen(2)
    N, H, W, Cn = shape
    K = 7
    p, w, b = torch.randn(shape, generator=g, dtype=D), torch.randn(K * K, Cn, generator=g, dtype=D), torch.randn(1, generator=g, dtype=D)
    dy = torch.randn(N, H, W, generator=g, dtype=D)
    dw0, db0 = torch.randn(K * K, Cn, generator=g, dtype=D), torch.randn(1, generator=g, dtype=D)
    pt, wt, bt = (t.clone().requires_grad_(True) for t in (p, w, b))
    y = F.conv2d(nchw(pt), wt.view(K, K, Cn).permute(2, 0, 1).unsqueeze(0).contiguous(), bt, padding=K // 2)[:, 0]
    ref, sa = BR.fpa_in_fwd(p, w, b, K)
    close(ref, y.detach())
    assert bool((sa >= ref.abs() - 1e-12).all())
    (y * dy).sum().backward()
    r = BR.fpa_in_bwd(p, dy, w, dw0, db0, K)
    close(r['dp'][0], pt.grad)
    close(r['dw'][0], wt.grad + dw0)
    close(r['db'][0], bt.grad + db0)
    for k in r:
        assert bool((r[k][1] >= r[k][0].abs() - 1e-12).all())


@pytest.mark.parametrize('K', [3, 5, 7])
def test_pyramid_phase_references_match_torch(K):
    g = R.gen(3 + K)
    x = torch.randn(3, 11, 7, generator=g, dtype=D)
    w, b = torch.randn(K * K, generator=g, dtype=D), torch.randn(1, generator=g, dtype=D)
    close(BR.pyr_conv(x, w, b, K)[0], F.conv2d(x.unsqueeze(1), w.view(1, 1, K, K), b, padding=K // 2)[:, 0])
    # BatchNorm2d(1) with batch statistics: output, and the running statistics (the UNBIASED variance goes into running_var)
    gamma, beta = torch.tensor([1.3], dtype=D), torch.tensor([-0.2], dtype=D)
    rm, rv = torch.tensor([0.4], dtype=D), torch.tensor([1.7], dtype=D)
    want = F.batch_norm(x.unsqueeze(1), rm, rv, gamma, beta, True, BR.BN_MOM, BR.BN_EPS)[:, 0]
    mean, var, unb, _ = BR.pyr_bn_stats(x)
    z, out, mag = BR.pyr_bn_relu_out(x, mean, 1.0 / torch.sqrt(var + BR.BN_EPS), gamma[0], beta[0])
    close(z, want)
    close(out, F.relu(want))
    assert bool((mag >= z.abs() - 1e-12).all())
    close(rm, (0.9 * 0.4 + 0.1 * mean).view(1))
    close(rv, (0.9 * 1.7 + 0.1 * unb).view(1))
    assert float((unb - var).abs()) > 1e-3 * float(var)      # the two variances are told apart at this size
    # eval: running statistics
    want = F.batch_norm(x.unsqueeze(1), rm, rv, gamma, beta, False, 0.0, BR.BN_EPS)[:, 0]
    close(BR.pyr_bn_relu_out(x, rm[0], 1.0 / torch.sqrt(rv[0] + BR.BN_EPS), gamma[0], beta[0])[0], want)


@pytest.mark.parametrize('sizes', [((1, 1), (2, 2)), ((2, 1), (5, 3)), ((5, 3), (11, 7)), ((11, 7), (22, 14)), ((2, 3), (4, 6)), ((4, 6), (8, 12))])
def test_bilinear_reference_matches_interpolate(sizes):
    (ih, iw), (oh, ow) = sizes
    x = torch.randn(2, ih, iw, generator=R.gen(4), dtype=D)
    ref, mag = BR.pyr_resize(x, oh, ow)
    want = F.interpolate(x.unsqueeze(1), size=(oh, ow), mode='bilinear', align_corners=True)[:, 0]
    close(ref, want, 2e-6)       # (the weights are float32 numbers, as in the kernel)
    assert bool((mag >= ref.abs() - 1e-12).all())
    i0, i1, l = BR.bil_coord(ih, oh)
    assert l.dtype == torch.float32 and bool((l >= 0).all()) and bool((l < 1).all()) and int(i1.max()) <= ih - 1


def test_mix_softmax_and_gather_references_match_torch():
    g = R.gen(5)
    N, HW, Cn = 2, 6, 8
    uu, mid, b1, gg = (torch.randn(s, generator=g, dtype=D) for s in ((N, HW), (N, HW, Cn), (N, Cn), (N, HW, Cn)))
    ut, mt = uu.clone().requires_grad_(True), mid.clone().requires_grad_(True)
    out = ut.unsqueeze(-1) * mt + b1.unsqueeze(1)
    close(BR.fpa_mix_fwd(uu, mid, b1)[0], out.detach())
    (out * gg).sum().backward()
    (dm, _), (du, dua) = BR.fpa_mix_bwd(uu, mid, gg)
    close(dm, mt.grad)
    close(du, ut.grad)
    assert bool((dua >= du.abs() - 1e-12).all())
    # softmax over the flattened map and its gradient
    S = (torch.randn(2, 81, generator=g, dtype=D) * 50).requires_grad_(True)
    P = torch.softmax(S, dim=1)
    close(BR.pab_softmax_fwd(S.detach()), P.detach())
    dP = torch.randn(2, 81, generator=g, dtype=D)
    (P * dP).sum().backward()
    ref, mag = BR.pab_softmax_bwd(dP, P.detach())
    close(ref, S.grad)
    assert bool((mag >= ref.abs() - 1e-15).all())
    # the un-transposed reshape
    x = torch.randn(N, HW, Cn, generator=g, dtype=D)
    M = torch.randn(N, HW * Cn, generator=g, dtype=D).requires_grad_(True)
    y = x.transpose(1, 2) + M.reshape(N, Cn, HW)
    close(BR.pab_mix_fwd(x, M.detach())[0], y.detach().transpose(1, 2))
    dy = torch.randn(N, HW, Cn, generator=g, dtype=D)
    (y.transpose(1, 2) * dy).sum().backward()
    close(BR.pab_mix_bwd(dy), M.grad)


@pytest.mark.parametrize('hw,Cn', BC.GEMM_SHAPES)
def test_gemm_stride_sets_match_matmul_and_autograd(hw, Cn):
    """The six named stride sets, composed as the plan composes them, give autograd's gradients of the torch PAB."""
    g = R.gen(6)
    N = 2
    x, bottom, dy = (torch.randn(N, hw, Cn, generator=g, dtype=D) for _ in range(3))
    center, top = (torch.randn(N, hw, 64, generator=g, dtype=D) * 0.2 for _ in range(2))
    ct, tt, bt = (t.clone().requires_grad_(True) for t in (center, top, bottom))
    y, S, P, M = BR.pab_torch(x, ct, tt, bt)
    (y * dy).sum().backward()
    G = {k: f(hw, Cn) for k, f in B.GEMMS.items()}
    run = lambda k, A, Bm: BR.pab_gemm(G[k], N, A, Bm)[0]      # noqa: E731
    rS = run('S', center, top)
    close(rS.view(N, hw, hw), S.detach())
    rP = BR.pab_softmax_fwd(rS.view(N, -1))
    rM = run('M', rP, bottom)
    close(rM.view(N, hw, Cn), M.detach())
    close(BR.pab_mix_fwd(x, rM.view(N, -1))[0], y.detach())
    dM = BR.pab_mix_bwd(dy)
    dPr = run('dP', dM, bottom)
    close(run('dbottom', rP, dM).view(N, hw, Cn), bt.grad)
    dS = BR.pab_softmax_bwd(dPr.view(N, -1), rP)[0]
    close(run('dcenter', dS, top).view(N, hw, 64), ct.grad)
    close(run('dtop', dS, center).view(N, hw, 64), tt.grad)
    # accum: the reference adds what is there, and counts it in the sum of magnitudes
    C0 = torch.randn(N * hw * hw, generator=g, dtype=D)
    ref, sa = BR.pab_gemm(G['S'], N, center, top, C0)
    close(ref, rS + C0)
    assert bool((sa >= ref.abs() - 1e-12).all())
    # every flat C element of every set is written exactly once (no NaN left in the reference)
    for k, gm in G.items():
        assert gm.numelC == gm.M * gm.N and gm.numelA == gm.M * gm.K and gm.numelB == gm.K * gm.N, k


def test_restated_pyramid_and_pab_match_the_oracle_blocks():
    torch.manual_seed(0)
    N, Cn, h, w, Co = 3, 6, 22, 14, 4
    blk = nets.FPABlock(Cn, Co).double().train()
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, torch.nn.BatchNorm2d):
                m.weight.uniform_(0.7, 1.3)
                m.bias.uniform_(-0.1, 0.5)
    x = torch.randn(N, Cn, h, w, dtype=D)
    layers = [blk.down1[1], blk.down2[1], blk.down3[1], blk.down3[2], blk.conv2, blk.conv1]
    prm = dict(hw=(h, w), w=[l.conv.weight.detach().reshape(-1) for l in layers], b=[l.conv.bias.detach() for l in layers],
               gamma=[l.bn.weight.detach() for l in layers], beta=[l.bn.bias.detach() for l in layers])
    with torch.no_grad():
        x1raw = layers[0].conv(F.max_pool2d(x, 2, 2))[:, 0]
        mid = blk.mid(x)
        b1 = blk.branch1(x)
        out = blk(x)
    uu, it = BR.pyramid_torch(x1raw, prm)
    close(uu.unsqueeze(1) * mid + b1, out, 1e-10)
    # the chain reference from the block's input on: the same forward (NHWC operands)
    xs = x.permute(0, 2, 3, 1).contiguous()
    w0 = layers[0].conv.weight.detach()[0].permute(1, 2, 0).reshape(49, Cn)
    res, _, out2 = BR.fpa_block_grads(xs, w0, layers[0].conv.bias.detach(), prm, mid.flatten(2).transpose(1, 2), b1[:, :, 0, 0],
                                      torch.ones(N, h * w, Co, dtype=D))
    close(out2, out.flatten(2).transpose(1, 2), 1e-10)
    assert res['dx'].shape == xs.shape and res['dw0'].numel() == 49 * Cn
    # the teacher-forced phase references, chained, give the same uu
    v = {}
    v['x1'] = BR.pyr_bn_relu_out(x1raw, *_ms(x1raw), prm['gamma'][0][0], prm['beta'][0][0])[1]

    def cbr(src, l):
        raw = BR.pyr_conv(src, prm['w'][l], prm['b'][l], BR.PYR_K[l])[0]
        return BR.pyr_bn_relu_out(raw, *_ms(raw), prm['gamma'][l][0], prm['beta'][l][0])[1]
    x2 = cbr(BR.pyr_maxpool(v['x1']), 1)
    x3 = cbr(cbr(BR.pyr_maxpool(x2), 2), 3)
    t = cbr(x2, 4) + BR.pyr_resize(x3, h // 4, w // 4)[0]
    u = BR.pyr_resize(t, h // 2, w // 2)[0] + cbr(v['x1'], 5)
    close(BR.pyr_resize(u, h, w)[0], uu, 1e-5)
    # PAB
    pab = nets.PAB(Cn, Cn).double()
    seen = []
    pab.out_conv.register_forward_pre_hook(lambda m, a: seen.append(a[0].detach()))
    xp = torch.randn(2, Cn, 4, 5, dtype=D)
    with torch.no_grad():
        pab(xp)
        fl = lambda t: t.flatten(2).transpose(1, 2)      # noqa: E731
        y, _, _, _ = BR.pab_torch(fl(xp), fl(pab.center_conv(xp)), fl(pab.top_conv(xp)), fl(pab.bottom_conv(xp)))
    close(y, fl(seen[0]), 1e-12)


def _ms(raw):
    mean, var, _, _ = BR.pyr_bn_stats(raw)
    return mean, 1.0 / torch.sqrt(var + BR.BN_EPS)


# ------------------------------------------------------------------------------------------------ Rule X inputs are exact
@pytest.mark.parametrize('family', sorted(BC.FAMILIES))
def test_rule_x_input_sets_are_exact(family):
    """Evaluated in float32 and in float64 the references agree, and what is stored as T is a float32 already."""
    seen = 0
    for case in BC.FAMILIES[family]():
        if case.refs is None:
            continue
        r64 = case.refs()
        with R.as_float32():
            r32 = case.refs()
        assert set(r64) == set(r32) and r64
        for k in r64:
            a, b = r32[k].to(r64[k].dtype), r64[k]
            assert torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0)), f'{case.id}: {k} differs between float32 and float64'
            shape = case.outs[k][0] if k in case.outs else tuple(case.ins[k].shape)
            assert r64[k].numel() == torch.Size(shape).numel(), f'{case.id}: {k}'
            assert R.is_f32_exact(r64[k]) and not bool(torch.isnan(r64[k]).any()), f'{case.id}: {k} is not a float32'
        seen += 1
    exact_families = {'maxpool2', 'fpa_in', 'fpa_mix', 'pab_gemm', 'pab_softmax', 'pab_mix'}
    assert (seen > 0) == (family in exact_families), (family, seen)


def test_case_table_respects_the_size_limits():
    ids = set()
    for fam, fn in BC.FAMILIES.items():
        for case in fn():
            assert case.id not in ids, case.id
            ids.add(case.id)
    assert all(max(s[1:3]) <= 22 and s[3] <= 264 for s in BC.MAXPOOL_SHAPES + BC.IN_SHAPES) and all(max(s[1:]) <= 24 for s in BC.PYR_SHAPES)
    assert all(h // 2 <= 22 and w // 2 <= 22 for _, h, w in BC.PYR_SHAPES)      # (the pyramid's own maps; the block's map is twice that)


# ------------------------------------------------------------------------------------------------ the pyramid seeds: no kink within 1e-3
@pytest.mark.parametrize('shape', BC.PYR_SHAPES + (BC.CHAIN[:3],))
def test_kink_margins_of_the_pyramid_seeds(shape):
    """In the float64 reference every BatchNorm output in front of a ReLU has |z| >= 1e-3 and every max-pool window with a positive winner
    leads its runner-up by >= 1e-3, so the gradient is differentiable at the tested point and no element needs excluding."""
    N, h, w = shape
    if shape == BC.CHAIN[:3]:
        its = [BR.fpa_block_grads(*BC.chain_inputs(T), torch.float64, T)[1] for T in BC.TRAIN_DTYPES]
    else:
        x1raw, prm, duu = BC.pyr_inputs(N, h, w, BC.PYR_SEED[shape])
        its = [BR.pyramid_grads(x1raw, prm, duu)[1]]
    for it in its:
        zmin, lead = BR.kink_margins(it)
        assert zmin >= BC.KINK, f'{shape}: |z| comes within {zmin:.2e} of a ReLU kink'
        assert lead >= BC.KINK, f'{shape}: a max-pool winner leads by {lead:.2e} only'
        off = BR.unit_off_fractions(it)
        assert 0.05 <= off['z_down1'] <= 0.95 and 0.05 <= off['z_down2'] <= 0.95, off


# ------------------------------------------------------------------------------------------------ layouts and wrappers
@pytest.mark.parametrize('shape', BC.PYR_SHAPES + ((1, 8, 9), (2, 31, 17)))
def test_scratch_layouts_match_the_library(shape):
    lib = L.lib()
    N, h, w = shape
    assert B.fpa_scratch_floats(N, h, w) == lib.octseg_fpa_scratch_floats(N, h, w)
    assert B.fpa_gscratch_floats(N, h, w) == lib.octseg_fpa_gscratch_floats(N, h, w)
    assert B.fpa_uu_offset(N, h, w) == lib.octseg_fpa_uu_offset(N, h, w)
    v = B.fpa_scratch_views(N, h, w)
    assert list(v) == ['r1', 'x1', 'c1', 'y1', 'tu', 'p2', 'r2', 'x2', 'c2', 'y2', 'x3u', 't', 'p3', 'r3a', 'x3a', 'r3b', 'x3', 'uu', 'stats', 'spare']
    assert v['r1'][0] == 0 and v['uu'] == (B.fpa_uu_offset(N, h, w), (N, h, w)) and v['stats'][0] == v['uu'][0] + N * h * w
    gv = B.fpa_gscratch_views(N, h, w)
    assert gv['dx1'][0] == N * (h // 2) * (w // 2)        # d x1raw: what plan_backward.cpp hands to fpa_in_bwd (gs + n1)
    s = torch.arange(B.fpa_scratch_floats(N, h, w), dtype=torch.float32)
    tv = B.fpa_scratch_views(N, h, w, s)
    assert tv['x2'].shape == (N, h // 4, w // 4) and float(tv['x2'].reshape(-1)[0]) == v['x2'][0]
    assert lib.octseg_fpa_scratch_floats(2, 7, 16) == 0 and lib.octseg_fpa_scratch_floats(0, 8, 8) == 0


def test_wrappers_check_buffer_extents_before_the_call():
    z = torch.zeros
    with pytest.raises(AssertionError):
        B.maxpool2_fwd(z(1, 4, 4, 8), z(1, 2, 2, 4))
    with pytest.raises(AssertionError):
        B.maxpool2_bwd(z(1, 4, 4, 8), z(1, 2, 2, 8), z(1, 4, 4, 4), 0)
    with pytest.raises(AssertionError):
        B.fpa_in_fwd(z(1, 4, 4, 8), z(49, 4), z(1), z(1, 4, 4))
    with pytest.raises(AssertionError):
        B.fpa_in_bwd(z(1, 4, 4, 8), z(1, 4, 3), z(49, 8), z(1, 4, 4, 8), z(49, 8), z(1))
    with pytest.raises(AssertionError):
        B.fpa_in_fwd(z(1, 4, 4, 8), z(49, 8), z(1), z(1, 4, 4, dtype=torch.float64))
    prm = dict(w=[None] + [z(k * k) for k in B.PYR_K[1:]], b=[None] + [z(1)] * 5, gamma=[z(1)] * 6, beta=[z(1)] * 6, rm=[z(1)] * 6, rv=[z(1)] * 6)
    with pytest.raises(AssertionError):
        B.fpa_pyr_fwd(z(B.fpa_scratch_floats(2, 8, 8) - 1), prm, 2, 8, 8, 1)
    bad = dict(prm, w=[None] + [z(9)] * 5)
    with pytest.raises(AssertionError):
        B.fpa_pyr_fwd(z(B.fpa_scratch_floats(2, 8, 8)), bad, 2, 8, 8, 1)
    with pytest.raises(AssertionError):
        B.fpa_pyr_fwd(z(64), prm, 2, 7, 8, 1)
    with pytest.raises(AssertionError):
        B.fpa_mix_fwd(z(2, 5), z(2, 6, 8), z(2, 8), z(2, 6, 8))
    with pytest.raises(AssertionError):
        B.fpa_mix_bwd(z(2, 6), z(2, 6, 8), z(2, 6, 8), z(2, 6, 8), z(2, 5))
    gm = B.gemm_M(9, 8)
    with pytest.raises(AssertionError):
        B.pab_gemm(gm, z(2 * 81), z(2 * 9 * 8 - 1), z(2 * 72), 2, dtype=L.F32)
    with pytest.raises(AssertionError):      # P is float32 scratch whatever the dtype
        B.pab_gemm(gm, z(2 * 81, dtype=torch.bfloat16), z(2 * 72, dtype=torch.bfloat16), z(2 * 72), 2)
    with pytest.raises(AssertionError):
        B.pab_softmax_bwd(z(2, 81), z(2, 80))
    with pytest.raises(AssertionError):
        B.pab_mix_fwd(z(2, 6, 8), z(2, 47), z(2, 6, 8))
    with pytest.raises(AssertionError):
        B.pab_mix_bwd(z(2, 6, 8), z(2, 6, 8, dtype=torch.float64).view(2, 48))


# ------------------------------------------------------------------------------------------------ refusals (host side, no launch)
A = 0x10000      # an aligned address that is never dereferenced: every call below is refused before any launch
OK, BAD_SHAPE, BAD_DTYPE, BAD_ARG = 0, -1, -2, -5


def _fpa(**kw):
    base = dict(N=2, H=8, W=8, C=8, K=7, train=1, accum=0, x=A, p=A, dp=A, dx=A, w=A, b=A, y=A, dy=A, dw=A, db=A, scratch=A, scratch_floats=1 << 20, gscratch=A,
                gscratch_floats=1 << 20, uu=A, duu=A, mid=A, b1=A, out=A, g=A, dmid=A)
    arrays = {k: [A] * 6 for k in ('pw', 'pb', 'pg', 'pbe', 'prm', 'prv', 'pdw', 'pdb', 'pdg', 'pdbe')}
    for k in list(kw):
        if k in arrays:
            arrays[k] = kw.pop(k)
    base.update(kw)
    d = L.FpaDesc(**base)
    for k, v in arrays.items():
        for l in range(6):
            getattr(d, k)[l] = v[l]
    return d


def _lack(d6, l):
    v = [A] * 6
    v[l] = None
    return v


def test_fpa_op_refusals():
    lib = L.lib()
    err = lib.octseg_last_error
    rc = lambda stage, dt=L.F32, **kw: B.fpa_op_raw(stage, dt, _fpa(**kw))      # noqa: E731
    assert B.fpa_op_raw(len(B.FPA_STAGES), L.F32, _fpa()) == BAD_ARG and B.fpa_op_raw(-1, L.F32, _fpa()) == BAD_ARG and b'unknown stage' in err()
    assert B.fpa_op_raw('in_fwd', L.F32, None) == BAD_ARG and b'null descriptor' in err()
    for stage in B.FPA_STAGES:
        assert rc(stage, 7) == BAD_DTYPE
        if stage.endswith('_bwd'):
            assert rc(stage, L.F16) == BAD_DTYPE and b'f16' in err(), stage
        assert rc(stage, N=0) == BAD_SHAPE and rc(stage, H=0) == BAD_SHAPE, stage
    # maxpool2: whole vectors, even maps, 16-byte alignment, null pointers
    assert rc('maxpool2_fwd', C=6) == BAD_SHAPE and rc('maxpool2_fwd', L.BF16, C=12) == BAD_SHAPE and rc('maxpool2_fwd', L.F16, C=4) == BAD_SHAPE
    assert rc('maxpool2_bwd', L.BF16, C=4) == BAD_SHAPE and rc('maxpool2_fwd', C=0) == BAD_SHAPE
    assert rc('maxpool2_fwd', H=7) == BAD_SHAPE and rc('maxpool2_bwd', W=5) == BAD_SHAPE and b'odd' in err()
    assert rc('maxpool2_fwd', x=None) == BAD_ARG and rc('maxpool2_fwd', p=None) == BAD_ARG and b'null' in err()
    assert rc('maxpool2_bwd', dp=None) == BAD_ARG and rc('maxpool2_bwd', dx=None) == BAD_ARG and rc('maxpool2_bwd', x=None) == BAD_ARG
    assert rc('maxpool2_fwd', x=A + 8) == BAD_ARG and rc('maxpool2_fwd', p=A + 4) == BAD_ARG and b'16-byte' in err()
    assert rc('maxpool2_bwd', L.BF16, dp=A + 2) == BAD_ARG and rc('maxpool2_bwd', dx=A + 8) == BAD_ARG
    assert rc('maxpool2_fwd', N=1 << 15, H=1 << 10, W=1 << 10) == BAD_SHAPE and b'2^31' in err()
    # the wide conv: K, nulls, element alignment
    assert rc('in_fwd', K=4) == BAD_SHAPE and rc('in_fwd', K=0) == BAD_SHAPE and rc('in_bwd', K=17) == BAD_SHAPE and rc('in_fwd', C=0) == BAD_SHAPE
    for k in ('p', 'w', 'b', 'y'):
        assert rc('in_fwd', **{k: None}) == BAD_ARG, k
    for k in ('p', 'w', 'dy', 'dp', 'dw', 'db'):
        assert rc('in_bwd', **{k: None}) == BAD_ARG, k
    assert rc('in_fwd', w=A + 2) == BAD_ARG and b'aligned' in err() and rc('in_fwd', p=A + 2) == BAD_ARG and rc('in_fwd', L.BF16, p=A + 1) == BAD_ARG
    assert rc('in_bwd', dy=A + 1) == BAD_ARG and rc('in_bwd', L.BF16, dp=A + 1) == BAD_ARG and rc('in_bwd', db=A + 2) == BAD_ARG
    # the pyramid: map, training batch, scratch sizes, nulls
    for stage in ('pyr_fwd', 'pyr_bwd'):
        assert rc(stage, H=7) == BAD_SHAPE and rc(stage, W=4) == BAD_SHAPE and b'H / 8' in err(), stage
        assert rc(stage, N=1, H=8, W=15) == BAD_SHAPE and b'Expected more than 1 value per channel when training, got input size torch.Size([1, 1, 1, 1])' in err()
        assert rc(stage, scratch=None) == BAD_ARG and rc(stage, scratch=A + 2) == BAD_ARG
        assert rc(stage, scratch_floats=lib.octseg_fpa_scratch_floats(2, 8, 8) - 1) == BAD_ARG and b'fpa_pyr_scratch_floats' in err()
        assert rc(stage, pg=_lack('pg', 3)) == BAD_ARG and rc(stage, pw=_lack('pw', 1)) == BAD_ARG and rc(stage, pw=[A + 1] * 6) == BAD_ARG
    with pytest.raises(ValueError, match='Expected more than 1 value per channel'):
        L.check(rc('pyr_fwd', N=1, H=8, W=8))
    for k in ('pb', 'pbe', 'prm', 'prv'):
        assert rc('pyr_fwd', **{k: _lack(k, 5)}) == BAD_ARG, k
    for k in ('pdw', 'pdb', 'pdg', 'pdbe'):
        assert rc('pyr_bwd', **{k: _lack(k, 2)}) == BAD_ARG, k
    assert rc('pyr_bwd', gscratch=None) == BAD_ARG and rc('pyr_bwd', duu=None) == BAD_ARG and rc('pyr_bwd', duu=A + 3) == BAD_ARG
    assert rc('pyr_bwd', gscratch_floats=lib.octseg_fpa_gscratch_floats(2, 8, 8) - 1) == BAD_ARG and b'gscratch' in err()
    # the mix
    assert rc('mix_fwd', C=0) == BAD_SHAPE
    for k in ('uu', 'mid', 'b1', 'out'):
        assert rc('mix_fwd', **{k: None}) == BAD_ARG, k
    for k in ('uu', 'mid', 'g', 'dmid', 'duu'):
        assert rc('mix_bwd', **{k: None}) == BAD_ARG, k
    assert rc('mix_fwd', uu=A + 2) == BAD_ARG and rc('mix_fwd', L.F16, out=A + 1) == BAD_ARG and rc('mix_bwd', mid=A + 2) == BAD_ARG


def _gemm(gm=None, batch=2, numel=None, **kw):
    gm = gm or B.gemm_S(9, 8)
    d = B.gemm_desc(gm, batch, A, A, A, 0, numel)
    for k, v in kw.items():
        setattr(d.gemm, k, v)
    return d


def test_pab_op_refusals():
    lib = L.lib()
    err = lib.octseg_last_error
    assert B.pab_op_raw(len(B.PAB_STAGES), L.F32, _gemm()) == BAD_ARG and B.pab_op_raw(-1, L.F32, _gemm()) == BAD_ARG and b'unknown stage' in err()
    assert B.pab_op_raw('gemm', L.F32, None) == BAD_ARG
    soft = lambda **kw: L.PabDesc(**dict(dict(S=A, P=A, batch=2, n=81), **kw))      # noqa: E731
    mix = lambda **kw: L.PabDesc(**dict(dict(x=A, M=A, y=A, dM=A, dy=A, N=2, HW=6, C=8), **kw))      # noqa: E731
    for stage, d in (('gemm', _gemm()), ('softmax_fwd', soft()), ('softmax_bwd', soft()), ('mix_fwd', mix()), ('mix_bwd', mix())):
        assert B.pab_op_raw(stage, 5, d) == BAD_DTYPE, stage
    assert B.pab_op_raw('softmax_bwd', L.F16, soft()) == BAD_DTYPE and B.pab_op_raw('mix_bwd', L.F16, mix()) == BAD_DTYPE and b'f16' in err()
    g = lambda dt=L.F32, **kw: B.pab_op_raw('gemm', dt, _gemm(**kw))      # noqa: E731
    # every named stride set reaches exactly its buffers: one element fewer in A, B or C is refused
    for name, make in B.GEMMS.items():
        for hw, Cn in BC.GEMM_SHAPES:
            gm = make(hw, Cn)
            full = [2 * gm.numelA, 2 * gm.numelB, 2 * gm.numelC]
            for i, what in enumerate((b'of A', b'of B', b'of C')):
                short = list(full)
                short[i] -= 1
                assert B.pab_op_raw('gemm', L.BF16, _gemm(gm, numel=short)) == BAD_SHAPE and what in err(), (name, hw, i)
    assert g(M=10) == BAD_SHAPE and g(N=10) == BAD_SHAPE and g(K=65) == BAD_SHAPE and g(numel=(3 * 576, 3 * 576, 3 * 81 - 1), batch=3) == BAD_SHAPE and g(sAm=65) == BAD_SHAPE and g(sCn=2) == BAD_SHAPE
    assert g(M=0) == BAD_SHAPE and g(K=0) == BAD_SHAPE and g(batch=0) == BAD_SHAPE
    assert B.pab_op_raw('gemm', L.F32, _gemm(batch=65536, numel=(1 << 40,) * 3)) == BAD_SHAPE and b'65535' in err()
    assert g(A=None) == BAD_ARG and g(B=None) == BAD_ARG and g(C=None) == BAD_ARG and b'null' in err()
    assert g(A=A + 2) == BAD_ARG and g(L.BF16, A=A + 1) == BAD_ARG and g(L.BF16, C=A + 2) == BAD_ARG and b'aligned' in err()      # (C of S is float32 scratch)
    assert g(sAb=1 << 31) == BAD_SHAPE
    # softmax
    s = lambda stage='softmax_fwd', dt=L.F32, **kw: B.pab_op_raw(stage, dt, soft(**kw))      # noqa: E731
    assert s(n=0) == BAD_SHAPE and b'n == 0' in err() and s(batch=0) == BAD_SHAPE and s(batch=65536) == BAD_SHAPE and b'65535' in err()
    assert s(n=1 << 31) == BAD_SHAPE and s(S=None) == BAD_ARG and s('softmax_bwd', P=None) == BAD_ARG and s(S=A + 2) == BAD_ARG and s('softmax_bwd', P=A + 1) == BAD_ARG
    # mix
    m = lambda stage='mix_fwd', dt=L.F32, **kw: B.pab_op_raw(stage, dt, mix(**kw))      # noqa: E731
    assert m(N=0) == BAD_SHAPE and m(HW=0) == BAD_SHAPE and m(C=0) == BAD_SHAPE and m(N=1 << 12, HW=1 << 12, C=1 << 8) == BAD_SHAPE
    for k in ('x', 'M', 'y'):
        assert m(**{k: None}) == BAD_ARG, k
    assert m('mix_bwd', dy=None) == BAD_ARG and m('mix_bwd', dM=None) == BAD_ARG and m(x=A + 2) == BAD_ARG and m(dt=L.BF16, y=A + 1) == BAD_ARG and m('mix_bwd', dM=A + 2) == BAD_ARG
