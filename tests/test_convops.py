"""CPU side of the single-launch conv tests: the cases of tests/conv_cases.py are what they claim to be, before any GPU sees them.

  * every case takes the route it names (octseg_conv_layer_route on stand-in pointers: the query launches nothing and reads no memory)
  * exactness: for every exact case the float32 and the float64 evaluation of tests/conv_ref.py agree bit for bit, and each channel's
    sum |y| and sum y^2, counted in units of the products' granularity, stay below 2^24 -- so the slab sums are exact in any order too
  * coverage: every (forward route x fused feature) cell a route is eligible for has a case
  * the reference itself against torch.nn.functional and autograd on the materialised virtual input
  * two deliberately wrong references (padding that receives the affine; statistics of the rounded value) are told apart by the cases
  * the entry refuses, before any launch, what the launchers cannot take
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import conv_cases as CC
import conv_ref as CR
import sweep_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import convops as CO
from oct_segmentation_amd.convops import Layer, Src


def test_every_case_takes_the_route_it_names():
    ids = set()
    for c in CC.all_cases():
        assert c.id not in ids, f'duplicate case id {c.id}'
        ids.add(c.id)
        assert tuple(CO.route(c.mode, c.dt, c.layer, has=c.has)) == tuple(c.route), c.id


def reference(case, t, wrong=None):
    if case.mode == CC.FWD:
        return CR.forward(case.layer, t, case.T, case.rule, wrong)
    if case.mode == CC.DGRAD:
        return CR.backward_data(case.layer, t, case.T, case.rule)
    return CR.backward_weight(case.layer, t, case.T)


@pytest.mark.parametrize('group,T', [p for p in CC.GROUP_PARAMS if p[0] != 'rounding'], ids=[i for i in CC.GROUP_IDS if not i.startswith('rounding')])
def test_exact_cases_are_exact(group, T):
    for case in CC.group_cases(group, T):
        assert case.exact
        t = CC.make_operands(case)
        r64 = reference(case, t)
        with R.as_float32():
            r32 = reference(case, t)
        for k in r64:
            assert r32[k].dtype == torch.float32 and r64[k].dtype == torch.float64
            assert torch.equal(r32[k].to(torch.float64), r64[k]), f'{case.id} {k}: the float32 and float64 references differ'
        if case.mode == CC.FWD:
            g = CR.product_granularity(case.layer, t, case.T)
            y = r64['yf']
            s1 = float(y.abs().sum(dim=(0, 2, 3)).max()) / g
            s2 = float((y * y).sum(dim=(0, 2, 3)).max()) / (g * g)
            print(f'{case.id}: granularity {g}, max channel sum|y| = {s1:.0f} units, sum y^2 = {s2:.0f} units^2')
            assert s1 < 2 ** 24 and s2 < 2 ** 24, f'{case.id}: channel sums leave float32 ({s1:.3g}, {s2:.3g} units): thin the weights (nnz)'


def test_every_eligible_route_feature_cell_has_a_case():
    have = {}
    for c in CC.all_cases():
        if c.mode == CC.FWD and c.exact:
            for f in c.features:
                have.setdefault((c.route[0], f), []).append(c.id)
    missing = [(r, f) for r in CC.FORWARD_ROUTES for f in CC.FEATURES if (r, f) not in CC.INELIGIBLE and (r, f) not in have]
    assert not missing, f'no case for {missing}'
    # the one cell left out is left out by the code, not by this table: an `up` source takes a 1x1 layer off gemm1x1
    base = Layer(3, 8, 8, 1, 40, [Src(128, 1, True, True)])
    assert CO.route(CC.FWD, L.BF16, base) != ['gemm1x1']
    assert CO.route(CC.FWD, L.BF16, Layer(3, 8, 8, 1, 40, [Src(128, 0, True, True)])) == ['gemm1x1']
    # every padded case has a non-zero shift on every affine source
    for c in CC.all_cases():
        if c.exact and c.mode != CC.DGRAD and c.layer.pad and any(s.affine for s in c.layer.srcs):
            t = CC.make_operands(c)
            assert all(bool((t[f'shift{i}'] != 0).all()) for i, s in enumerate(c.layer.srcs) if s.affine), c.id


SMALL = [('mfma16', CC.BF16, 'decoder'), ('mfma16', CC.F32, 'stride2'), ('mfma16', CC.F32, 'convT'), ('mfma16', CC.F32, 'cat24_40'), ('gemm1x1', CC.BF16, 'ragged')]


def _materialised(case, t):
    """The virtual input as a leaf tensor [N][Cin][H][W] (float64, unpadded) and the weight as seen, for torch's own conv and autograd."""
    p = 0 if case.layer.transposed else case.layer.pad
    xp = CR.virtual_input(case.layer, t, case.T)
    x = xp[:, :, p:p + case.layer.H, p:p + case.layer.W].clone().requires_grad_(True)
    return x


def test_reference_matches_torch_functional_and_autograd():
    for group, T, name in SMALL:
        cases = [c for c in CC.group_cases(group, T) if c.name == name] + [c for c in CC.group_cases('wgrad', T) if c.name in ('9tap_s2', '4tap', 'decoder')]
        for case in cases:
            Ly = case.layer
            t = CC.make_operands(case)
            if case.mode == CC.DGRAD:      # the sources only say where the gradient goes: give the autograd graph an input
                for i in range(len(Ly.srcs)):
                    t[f'x{i}'] = torch.zeros(Ly.src_shape(i), dtype=case.T)
            if 'w' not in t:
                t['w'] = torch.zeros(Ly.w_shape)
            x = _materialised(case, t)
            w = CR.weight_as_seen(Ly, t, case.T, fold=case.mode == CC.FWD).clone().requires_grad_(True)
            if Ly.transposed:
                y = F.conv_transpose2d(x, w.permute(3, 2, 0, 1), stride=2, padding=1)
            else:
                y = F.conv2d(x, w.permute(2, 3, 0, 1), stride=Ly.stride, padding=Ly.pad)
            if case.mode == CC.FWD:
                if t.get('bias') is not None:
                    y = y + t['bias'].double().view(1, -1, 1, 1)
                assert torch.equal(y.detach(), CR.forward_f32value(Ly, t, case.T)), case.id
                continue
            dy = CR.nchw(CR.ref(t['dy']))
            gx, gw = torch.autograd.grad(y, (x, w), dy)
            if case.mode == CC.DGRAD:
                assert torch.equal(gx, CR.backward_data_full(Ly, t, case.T)), case.id
            else:
                assert torch.equal(gw, CR.backward_weight_terms(Ly, t, case.T)), case.id


def test_wrong_references_are_told_apart():
    """Padding filled with relu(shift), and statistics taken after the storage rounding: the exact cases see both."""
    seen_pad = seen_stats = 0
    for case in CC.group_cases('mfma16', CC.BF16) + CC.group_cases('thin', CC.BF16)[:2] + CC.group_cases('mfma11', CC.BF16):
        if case.mode != CC.FWD or not case.layer.pad or case.layer.transposed or 'slab' not in case.has:
            continue
        t = CC.make_operands(case)
        good = CR.forward(case.layer, t, case.T, case.rule)
        if any(s.affine for s in case.layer.srcs):
            bad = CR.forward(case.layer, t, case.T, case.rule, wrong='pad_affine')
            assert not torch.equal(good['y'], bad['y']) and not torch.equal(good['stats'], bad['stats']), f'{case.id}: a padding pixel with the affine goes unseen'
            # ... and only the border differs
            assert torch.equal(good['y'][:, 2:-2, 2:-2], bad['y'][:, 2:-2, 2:-2])
            seen_pad += 1
        bad = CR.forward(case.layer, t, case.T, case.rule, wrong='stats_rounded')
        assert torch.equal(good['y'], bad['y'])
        if not torch.equal(good['stats'], bad['stats']):
            seen_stats += 1
    assert seen_pad >= 5 and seen_stats >= 2, (seen_pad, seen_stats)


def test_store_rules_differ_where_the_value_is_not_representable():
    """'staged' rounds the value before it meets the old one, 'direct' does not: 37.125 + 0.25 in bf16 tells them apart (37.0 + 0.25 = 37.25 against 37.375 -> 37.5, ties to even)."""
    y = torch.tensor([[[[37.125, 2.0], [300.5, 1.0]]]], dtype=torch.float64)
    old = torch.tensor([[[[0.25, 1.0], [1.0, 1.0]]]], dtype=torch.float64)
    a, b = CR.store(y, old, CC.BF16, 1, 'staged'), CR.store(y, old, CC.BF16, 1, 'direct')
    assert a[0, 0, 0, 0] == 37.25 and b[0, 0, 0, 0] == 37.5 and torch.equal(a[0, 0, :, 1], b[0, 0, :, 1])
    assert float(CR.pool_store(y, None, CC.BF16, 0, 'staged')) == 340.0 and float(CR.pool_store(y, None, CC.BF16, 0, 'direct')) == 340.0


def test_accumulated_and_pooled_gradients_can_tell_the_store_rules_apart():
    """The data-gradient cases with an accumulated or pooled destination carry dense, positively biased operands (conv_cases.DENSE), so their values
    leave bf16's significand: each expects different tensors under the two store rules -- a route that rounded in the other order would fail."""
    n = 0
    for case in CC.all_cases():
        if case.mode != CC.DGRAD or case.T != CC.BF16 or not (any(case.layer.accum) or any(case.layer.pool)):
            continue
        t = CC.make_operands(case)
        a, b = CR.backward_data(case.layer, t, case.T, 'staged'), CR.backward_data(case.layer, t, case.T, 'direct')
        diff = sum(int((a[k] != b[k]).sum()) for k in a if k.startswith('dx'))
        assert diff >= 16, (case.id, diff)
        n += 1
    assert n >= 6, n


# ------------------------------------------------------------------------------------------------ refusals (nothing is launched: no GPU needed)
def _rc(mode, dt, layer, ptrs, nbytes=1 << 40):
    return CO.route_raw(mode, dt, CO.make_desc(layer, ptrs, nbytes))[0]


def test_entry_refuses_what_the_launchers_cannot_take():
    BAD_SHAPE, BAD_DTYPE, BAD_ARG = -1, -2, -5
    ok = Layer(2, 24, 40, 3, 16, [Src(32, 0, True, True)], pad=1)
    fp = lambda layer, mode=CC.FWD, has=(): CO.fake_ptrs(mode, layer, has)
    assert _rc(CC.FWD, L.BF16, ok, fp(ok)) == 0
    # pointers
    for k in ('x0', 'w', 'y', 'scratch', 'shift0'):
        p = fp(ok); del p[k]
        assert _rc(CC.FWD, L.BF16, ok, p) == BAD_ARG, k
    for k in ('x0', 'w', 'y', 'scale0'):
        p = fp(ok); p[k] += 8
        assert _rc(CC.FWD, L.BF16, ok, p) == BAD_ARG, k
        assert 'conv_layer_op' in L.lib().octseg_last_error().decode()
    assert _rc(CC.FWD, L.BF16, ok, fp(ok), nbytes=64) == BAD_ARG                                  # scratch smaller than the image
    # channels in whole 16-byte vectors
    assert _rc(CC.FWD, L.BF16, Layer(2, 24, 40, 3, 16, [Src(36)], pad=1), fp(Layer(2, 24, 40, 3, 16, [Src(36)], pad=1))) == BAD_SHAPE
    assert _rc(CC.FWD, L.F32, Layer(2, 24, 40, 3, 16, [Src(36)], pad=1), fp(Layer(2, 24, 40, 3, 16, [Src(36)], pad=1))) == 0
    assert _rc(CC.FWD, L.BF16, Layer(2, 24, 40, 3, 12, [Src(32)], pad=1), fp(ok)) == BAD_SHAPE
    six = Layer(1, 8, 8, 1, 16, [Src(8)] * 6)
    assert _rc(CC.FWD, L.BF16, six, CO.fake_ptrs(CC.FWD, Layer(1, 8, 8, 1, 16, [Src(8)] * 5))) == BAD_SHAPE
    odd = Layer(1, 9, 8, 3, 16, [Src(16, 1)], pad=1)                                                # 9 >> 1 = 4: 4 << 1 != 9
    assert _rc(CC.FWD, L.BF16, odd, fp(odd)) == BAD_SHAPE
    d = CO.make_desc(ok, fp(ok), 1 << 40); d.Cin = 40
    assert CO.route_raw(CC.FWD, L.BF16, d)[0] == BAD_SHAPE                                          # sum of C != Cin
    d = CO.make_desc(ok, fp(ok), 1 << 40); d.src[0].H = 23
    assert CO.route_raw(CC.FWD, L.BF16, d)[0] == BAD_SHAPE
    for bad in (Layer(1, 8, 8, 5, 16, [Src(16)], pad=2), Layer(1, 8, 8, 3, 16, [Src(16)], stride=3), Layer(1, 8, 8, 3, 16, [Src(16)], transposed=True),
                Layer(1, 8, 8, 3, 16, [Src(16)], pad=2)):
        assert _rc(CC.FWD, L.BF16, bad, fp(bad)) == BAD_SHAPE
    # the fused fields
    relu_only = Layer(1, 8, 8, 3, 16, [Src(16, 0, False, True)], pad=1)
    assert _rc(CC.FWD, L.BF16, relu_only, fp(relu_only)) == BAD_ARG
    ro = Layer(2, 24, 40, 3, 16, [Src(32)], pad=1, relu_out=True)
    assert _rc(CC.FWD, L.BF16, ro, fp(ro, has=('bias',))) == 0
    assert _rc(CC.FWD, L.BF16, ro, fp(ro)) == BAD_ARG                                               # relu_out without bias
    assert _rc(CC.FWD, L.BF16, ro, fp(ro, has=('bias', 'slab'))) == BAD_ARG                         # relu_out with the slab
    g1 = Layer(3, 7, 5, 1, 40, [Src(128)])
    assert CO.route(CC.FWD, L.BF16, g1, has=('slab',)) == ['gemm1x1']
    assert _rc(CC.FWD, L.BF16, g1, fp(g1, has=('bias', 'slab'))) == BAD_ARG                         # bias + slab on a gemm1x1 launch
    assert _rc(CC.FWD, L.F32, g1, fp(g1, has=('bias', 'slab'))) == 0                                # (f32 goes to conv_mfma: fine)
    hd = Layer(1, 24, 40, 3, 3, [Src(32)], pad=1, head=True)
    assert _rc(CC.FWD, L.BF16, hd, fp(hd, has=('bias',))) == 0
    assert _rc(CC.FWD, L.BF16, hd, fp(hd, has=('slab',))) == BAD_ARG                                # a slab in head mode
    hd.accum = (1, 0, 0, 0, 0)
    assert _rc(CC.FWD, L.BF16, hd, fp(hd)) == BAD_ARG
    # gradient modes
    assert _rc(CC.DGRAD, L.F16, ok, fp(ok, CC.DGRAD)) == BAD_DTYPE and _rc(CC.WGRAD, L.F16, ok, fp(ok, CC.WGRAD)) == BAD_DTYPE
    assert _rc(CC.FWD, 3, ok, fp(ok)) == BAD_DTYPE and _rc(3, L.BF16, ok, fp(ok)) == BAD_ARG
    plain = Layer(2, 24, 40, 3, 16, [Src(32)], pad=1)
    assert _rc(CC.DGRAD, L.BF16, plain, fp(plain, CC.DGRAD)) == 0 and _rc(CC.WGRAD, L.BF16, ok, fp(ok, CC.WGRAD)) == 0
    p = fp(plain, CC.DGRAD); p['bias'] = 0x1000
    assert _rc(CC.DGRAD, L.BF16, plain, p) == BAD_ARG                                                  # forward-only field
    pl = Layer(2, 24, 40, 3, 16, [Src(32)], pad=1, pool=(1, 0, 0, 0, 0))
    assert _rc(CC.DGRAD, L.BF16, pl, fp(pl, CC.DGRAD)) == BAD_ARG                                   # pool without an `up` source
    pl = Layer(2, 24, 40, 3, 16, [Src(32, 1)], stride=2, pad=1, pool=(1, 0, 0, 0, 0))
    assert _rc(CC.DGRAD, L.BF16, pl, fp(pl, CC.DGRAD)) == BAD_ARG                                   # pool at stride 2
    pl = Layer(2, 24, 40, 3, 16, [Src(32, 1)], pad=1, pool=(1, 0, 0, 0, 0))
    assert _rc(CC.DGRAD, L.BF16, pl, fp(pl, CC.DGRAD)) == 0
    assert _rc(CC.FWD, L.BF16, pl, fp(pl)) == BAD_ARG                                               # pool in a forward
    s2 = Layer(1, 8, 8, 1, 16, [Src(16)], stride=2)
    assert _rc(CC.DGRAD, L.BF16, s2, fp(s2, CC.DGRAD)) == BAD_ARG                                   # one parity only: the caller zeroes and accumulates
    s2.accum = (1, 0, 0, 0, 0)
    assert _rc(CC.DGRAD, L.BF16, s2, fp(s2, CC.DGRAD)) == 0
    assert CO.route(CC.DGRAD, L.BF16, s2) == ['mfma-16', None, None, None]
    p = fp(ok, CC.WGRAD); del p['dW']
    assert _rc(CC.WGRAD, L.BF16, ok, p) == BAD_ARG
    assert L.lib().octseg_conv_layer_route(0, 1, None, (C.c_int * 8)(), C.byref(C.c_int())) == BAD_ARG


def test_slab_rows_follow_the_routed_kernel():
    """One row per M tile of conv_mfma_kernel, per workgroup of the persistent kernels: the query wraps conv_num_mtiles_flat."""
    assert CO.slab_rows(L.F32, Layer(2, 24, 40, 3, 16, [Src(32)], pad=1)) == 2 * 3 * 3                  # 8 x 16-pixel tiles: 24 rows fill them whole
    assert CO.slab_rows(L.BF16, Layer(2, 33, 55, 3, 192, [Src(128)], pad=1)) == 2 * 3 * 5
    assert CO.slab_rows(L.BF16, Layer(4, 128, 128, 3, 136, [Src(128)], pad=1)) == 4 * 8 * 8
    rows_t = CO.slab_rows(L.BF16, Layer(1, 12, 20, 4, 16, [Src(32)], stride=2, pad=1, transposed=True))
    assert rows_t == 4 * 2 * 2                                                                           # four parity launches, each 8 x 16-pixel tiles over the 12 x 20 input grid
