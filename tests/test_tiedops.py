"""CPU side of the single-launch tests of the tied decoder layer: the cases of tests/tied_cases.py are what they claim to be.

  * every case takes the routes it names (octseg_tied_layer_route on stand-in pointers: nothing is launched), the table of shapes reaches the
    loops it is there for (masked 8x16, masked 11x11, the 16-tap stride-2 fallback; both sides of wgrad_convt16_eligible)
  * the reference against torch.nn.functional and autograd in float64: conv2d over interpolate(nearest) + cat
  * exactness: for every exact case the float32 and float64 evaluations agree bit for bit (so every partial sum stays below 2^24 units), and
    every 4x4 entry -- every sum of the taps that meet on one low-resolution pixel -- is a bf16; for the Gaussian weights too
  * the DENSE cases tell the tied store rules from the plain path's (pooled quads; the sum rounded once)
  * every refusal of the door, and the extent arithmetic of the wrapper
tests/test_tied_identity.py (the algebra of the decomposition itself) stays what it is.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import conv_cases as CC
import conv_ref as CR
import sweep_ref as R
import tied_cases as TC
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import convops as CO
from oct_segmentation_amd.convops import Layer, Src

CASES = TC.all_cases()


def test_every_case_takes_the_routes_it_names():
    ids = set()
    for tc in CASES:
        assert tc.id not in ids, f'duplicate case id {tc.id}'
        ids.add(tc.id)
        c = tc.case
        assert tuple(CO.tied_route(c.mode, c.layer, wg_target=tc.wg_target)) == tuple(c.route), tc.id


def test_the_table_reaches_every_loop():
    S = TC.shapes()
    dg = {name: tuple(CO.tied_route(CC.DGRAD, mk())) for name, (mk, _) in S.items()}
    assert dg['m16_cs0'] == ('mfma-16-masked',) and dg['m16_cs32'] == ('mfma-16-masked', 'mfma-16')
    assert dg['m11'] == ('mfma-11-masked', 'mfma-16')
    assert dg['u32'] == ('mfma-16', 'mfma-16') and dg['u64'] == ('mfma-16',) and dg['skips2'][0] == 'mfma-16-masked'
    # the masked launch needs planes of whole K chunks: Cout a multiple of 64 (tie_images)
    assert CO.tied_route(CC.DGRAD, TC._layer(3, 6, 10, 96, [TC.up(64)])) == ['mfma-16']
    wr = TC.query_wroutes()
    assert wr['m16_cs32'] == ('convt16', 'mfma') and wr['m11'] == ('convt16', 'mfma') and wr['m16_cs0'] == ('convt16',), wr
    assert wr['w1tile'] == ('mfma',) * 5, wr           # the other side of wgrad_convt16_eligible: four parity launches + the skip slice
    for name, (mk, _) in S.items():
        Ly = mk()
        assert tuple(CO.tied_route(CC.FWD, Ly)) == TC.forward_routes(Ly)
        assert len(wr[name]) == (1 if wr[name][0] == 'convt16' else 4) + (1 if len(Ly.srcs) > 1 else 0)
    assert CO.side_wgs() == 144 and {tc.wg_target for tc in CASES} == {0, 144}


def _torch_layer(layer, t, T):
    """The layer as torch sees it: conv2d(cat(interpolate(x0, nearest x2), x1, ..), w, pad 1) on float64 leaves."""
    xs = []
    for i, s in enumerate(layer.srcs):
        x = CR.nchw(CR.ref(t[f'x{i}']))
        if s.affine:
            x = x * CR.ref(t[f'scale{i}']).view(1, -1, 1, 1) + CR.ref(t[f'shift{i}']).view(1, -1, 1, 1)
            x = CR.rnd(x.clamp_min(0) if s.relu else x, T)
        xs.append(x.clone().requires_grad_(True))
    cat = torch.cat([F.interpolate(x, scale_factor=2, mode='nearest') if s.up else x for x, s in zip(xs, layer.srcs)], dim=1)
    w = CR.weight_as_seen(layer, t, T).clone().requires_grad_(True)
    return xs, w, F.conv2d(cat, w.permute(2, 3, 0, 1), padding=1)


@pytest.mark.parametrize('name', ['m16_cs32', 'u32', 'skips2'])
def test_reference_matches_torch_functional_and_autograd(name):
    mk, droute = TC.shapes()[name]
    Ly = mk()
    tf = TC.make_operands(TC.Tied(TC._case(name, CC.FWD, Ly, (), nnz=9 * Ly.Cin // 2)))
    tg = TC.make_operands(TC.Tied(TC._case(name, CC.DGRAD, Ly, ())))
    t = {**tg, **tf}                                   # x, scale, shift, w of the forward; dy of the gradient
    xs, w, y = _torch_layer(Ly, t, TC.BF16)
    u, s = TC.forward_parts(Ly, t, TC.BF16)
    assert torch.equal(y.detach(), u + s)              # (exact operands: the split sum is the whole sum)
    grads = torch.autograd.grad(y, xs + [w], CR.nchw(CR.ref(t['dy'])))
    low, full = TC.backward_data_values(Ly, t, TC.BF16)
    assert torch.equal(grads[0], low), 'the low-resolution gradient is autograd\'s gradient of the stored source'
    c0 = Ly.srcs[0].C
    for i, sdesc in enumerate(Ly.srcs[1:], start=1):
        assert torch.equal(grads[i], full[:, c0:c0 + sdesc.C]), i
        c0 += sdesc.C
    tw = dict(t); tw['dW'] = torch.zeros(Ly.w_shape)
    assert torch.equal(grads[-1], TC.backward_weight(Ly, tw, TC.BF16)['dW'])


def _k4_sums(w):
    """Every sum of 3x3 taps that meets on one low-resolution pixel: rows A(u) x columns A(v), A(k) = [max(0, 2 - k), min(2, 3 - k)]; [4][4][O][I]."""
    A = [range(max(0, 2 - k), min(2, 3 - k) + 1) for k in range(4)]
    return torch.stack([torch.stack([sum(w[r, s] for r in A[u] for s in A[v]) for v in range(4)]) for u in range(4)])


def test_exact_cases_are_exact_and_every_4x4_entry_is_a_bf16():
    seen_gauss = 0
    for tc in CASES:
        c = tc.case
        t = TC.make_operands(tc)
        if 'w' in t:
            w64 = CR.weight_as_seen(c.layer, t, c.T).to(torch.float64)
            assert torch.equal(w64, t['w'].to(torch.float64)), f'{tc.id}: a weight is no bf16'
            k4 = _k4_sums(w64[..., :c.layer.srcs[0].C])
            assert torch.equal(k4.to(torch.float32).to(torch.float64), k4), f'{tc.id}: a float32 tap sum is inexact'
            assert torch.equal(k4.to(torch.float32).to(torch.bfloat16).to(torch.float64), k4), f'{tc.id}: a 4x4 entry is no bf16'
            seen_gauss += 0 if c.exact else 1
        if not c.exact:
            continue
        r64 = TC.reference(tc, t)
        with R.as_float32():
            r32 = TC.reference(tc, t)
        for k in r64:
            assert r32[k].dtype == torch.float32 and r64[k].dtype == torch.float64
            assert torch.equal(r32[k].to(torch.float64), r64[k]), f'{tc.id} {k}: the float32 and float64 references differ'
    assert seen_gauss >= 4
    A = [set(range(max(0, 2 - k), min(2, 3 - k) + 1)) for k in range(4)]
    assert A == [{2}, {1, 2}, {0, 1}, {0}]             # at most 2 x 2 = four taps per entry


def test_dense_cases_tell_the_store_rules_apart():
    n = 0
    for tc in CASES:
        c = tc.case
        if not c.exact or c.nnz != CC.DENSE or c.mode == CC.WGRAD:
            continue
        t = TC.make_operands(tc)
        good = TC.reference(tc, t)
        bad = TC.reference(tc, t, rule='whole' if c.mode == CC.FWD else 'pooled')
        key = 'y' if c.mode == CC.FWD else 'dx0'
        diff = int((good[key] != bad[key]).sum())
        print(f'{tc.id}: {diff} of {good[key].numel()} elements differ between the tied rule and the other one')
        if c.mode == CC.FWD or c.layer.accum[0]:
            assert diff >= 16, (tc.id, diff)
        n += 1
    assert n >= 8, n


# ------------------------------------------------------------------------------------------------ refusals (nothing is launched: no GPU needed)
def _rc(mode, layer, ptrs, dt=L.BF16, nbytes=1 << 40, wg=0):
    return CO.tied_route_raw(mode, dt, CO.make_desc(layer, ptrs, nbytes), wg)[0]


def test_entry_refuses_what_the_plan_would_not_build():
    BAD_SHAPE, BAD_DTYPE, BAD_ARG = -1, -2, -5
    ok = TC._layer(2, 12, 20, 64, [TC.up(72, CC.AR), CC.A(32)])
    fp = lambda layer, mode=CC.FWD: CO.fake_ptrs(mode, layer)
    for mode in (CC.FWD, CC.DGRAD, CC.WGRAD):
        assert _rc(mode, ok, fp(ok, mode)) == 0
        assert _rc(mode, ok, fp(ok, mode), dt=L.F32) == BAD_DTYPE and _rc(mode, ok, fp(ok, mode), dt=L.F16) == BAD_DTYPE
        assert _rc(mode, ok, fp(ok, mode), nbytes=CO.tied_scratch_bytes(ok) - 1) == BAD_ARG
        assert _rc(mode, ok, fp(ok, mode), nbytes=CO.tied_scratch_bytes(ok)) == 0
        assert _rc(mode, ok, fp(ok, mode), wg=-1) == BAD_ARG
        p = fp(ok, mode); del p['scratch']
        assert _rc(mode, ok, p) == BAD_ARG
        for k in CO.operand_names(mode, ok):
            p = fp(ok, mode); del p[k]
            assert _rc(mode, ok, p) == BAD_ARG, (mode, k)
            p = fp(ok, mode); p[k] += 8
            assert _rc(mode, ok, p) == BAD_ARG, (mode, k)
        assert 'tied_layer_op' in L.lib().octseg_last_error().decode()
        for k in ('wscale', 'slab'):
            assert _rc(mode, ok, {**fp(ok, mode), k: 0x900000}) == BAD_ARG, (mode, k)
        assert _rc(mode, ok, {**fp(ok, mode), 'bias': 0x900000}) == BAD_SHAPE          # (tie_eligible: the plan ties no biased layer)
    assert _rc(3, ok, fp(ok)) == BAD_ARG and _rc(CC.FWD, ok, fp(ok), dt=3) == BAD_DTYPE
    assert L.lib().octseg_tied_layer_route(0, L.BF16, None, 0, (C.c_int * 8)(), C.byref(C.c_int())) == BAD_ARG
    assert L.lib().octseg_tied_layer_route(0, L.BF16, C.byref(CO.make_desc(ok, fp(ok), 1 << 40)), 0, None, None) == BAD_ARG
    # layers the plan would not tie (tie_eligible)
    no = [
        TC._layer(2, 12, 20, 64, [TC.up(56), CC.P(32)]),                    # Ca below 64
        TC._layer(2, 12, 20, 64, [TC.up(72), CC.P(24)]),                    # a skip slice below 32
        TC._layer(2, 12, 20, 24, [TC.up(72), CC.P(32)]),                    # Cout below 32
        TC._layer(2, 12, 20, 64, [CC.P(72), CC.P(32)]),                     # src 0 not upsampled
        TC._layer(2, 12, 20, 64, [TC.up(72), TC.up(32)]),                   # an upsampled skip
        Layer(2, 24, 40, 1, 64, [TC.up(72)]),                               # not a 3x3
        Layer(2, 24, 40, 3, 64, [TC.up(72)], pad=0),
        Layer(2, 24, 40, 3, 64, [TC.up(72)], stride=2, pad=1),
        Layer(2, 12, 20, 4, 64, [TC.up(72)], stride=2, pad=1, transposed=True),
    ]
    for bad in no:
        assert _rc(CC.FWD, bad, fp(bad)) == BAD_SHAPE, bad
        assert L.lib().octseg_tied_layer_scratch_bytes(L.BF16, C.byref(CO.make_desc(bad, {}, 0))) == 0
    assert _rc(CC.FWD, TC._layer(2, 12, 20, 64, [TC.up(76)]), fp(ok)) == BAD_SHAPE                    # channels in whole vectors
    assert _rc(CC.FWD, TC._layer(2, 12, 20, 60, [TC.up(72)]), fp(ok)) == BAD_SHAPE
    d = CO.make_desc(ok, fp(ok), 1 << 40); d.Cin = 112
    assert CO.tied_route_raw(CC.FWD, L.BF16, d)[0] == BAD_SHAPE
    d = CO.make_desc(ok, fp(ok), 1 << 40); d.src[0].H = 11
    assert CO.tied_route_raw(CC.FWD, L.BF16, d)[0] == BAD_SHAPE
    d = CO.make_desc(ok, fp(ok), 1 << 40); d.head = 1
    assert CO.tied_route_raw(CC.FWD, L.BF16, d)[0] in (BAD_ARG, BAD_SHAPE)
    # the fused fields the tied passes do not carry
    ro = TC._layer(2, 12, 20, 64, [TC.up(72)]); ro.relu_out = True
    assert _rc(CC.FWD, ro, fp(ro)) == BAD_ARG
    sr = TC._layer(2, 12, 20, 64, [TC.up(72)]); sr.slab_row0 = 1
    assert _rc(CC.FWD, sr, fp(sr)) == BAD_ARG
    acc = TC._layer(2, 12, 20, 64, [TC.up(72)], (1, 0, 0, 0, 0))
    assert _rc(CC.FWD, acc, fp(acc)) == BAD_ARG and _rc(CC.DGRAD, acc, fp(acc, CC.DGRAD)) == 0          # accum belongs to the gradient
    pl = TC._layer(2, 12, 20, 64, [TC.up(72)]); pl.pool = (1, 0, 0, 0, 0)
    assert _rc(CC.DGRAD, pl, fp(pl, CC.DGRAD)) == BAD_ARG and _rc(CC.FWD, pl, fp(pl)) == BAD_ARG
    relu_only = TC._layer(2, 12, 20, 64, [Src(72, 1, False, True)])
    assert _rc(CC.FWD, relu_only, fp(relu_only)) == BAD_ARG
    p = fp(ok); del p['shift0']
    assert _rc(CC.FWD, ok, p) == BAD_ARG


def test_wrapper_derives_every_extent_from_the_layer():
    Ly = TC._layer(2, 11, 22, 128, [TC.up(136), CC.P(40)])
    assert (Ly.H, Ly.W, Ly.Cin) == (22, 44, 176) and Ly.src_shape(0) == (2, 11, 22, 136) and Ly.src_shape(1) == (2, 22, 44, 40)
    assert CO.tied_dst_shape(Ly, 0) == (2, 11, 22, 136) and CO.tied_dst_shape(Ly, 1) == (2, 22, 44, 40) and Ly.w_shape == (3, 3, 128, 176)
    # the scratch: job table + prefix sums, the four images, the f32 gradients of the 4x4 image and of the skip slice
    nb = CO.tied_scratch_bytes(Ly)
    assert nb >= 1024 + (16 * 136 + 9 * 40) * 128 * 4 + 2 * (16 * 136 + 9 * 40) * 128
    assert CO.tied_scratch_bytes(TC._layer(2, 11, 22, 128, [TC.up(136)])) < nb

    class FakeTensor:
        def __init__(self, shape, dtype):
            self.shape, self.dtype, self.is_cuda = torch.Size(shape), dtype, True

        def is_contiguous(self):
            return True

    bf, f32 = torch.bfloat16, torch.float32
    good = {'w': FakeTensor(Ly.w_shape, f32), 'dy': FakeTensor((2, 22, 44, 128), bf), 'dx0': FakeTensor((2, 11, 22, 136), bf), 'dx1': FakeTensor((2, 22, 44, 40), bf)}
    CO.check_tied_tensors(CC.DGRAD, Ly, good, bf)
    for k, v in (('dx0', FakeTensor((2, 22, 44, 136), bf)), ('dx1', FakeTensor((2, 11, 22, 40), bf)), ('dy', FakeTensor((2, 11, 22, 128), bf)),
                 ('w', FakeTensor((4, 4, 128, 176), f32)), ('dx0', FakeTensor((2, 11, 22, 136), f32))):
        with pytest.raises(AssertionError):
            CO.check_tied_tensors(CC.DGRAD, Ly, {**good, k: v}, bf)
    with pytest.raises(AssertionError):
        CO.check_tied_tensors(CC.DGRAD, Ly, {k: v for k, v in good.items() if k != 'dx1'}, bf)
