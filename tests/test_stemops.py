"""CPU side of the single-launch stem tests: the cases of tests/stem_cases.py are what they claim to be, before any GPU sees them.

  * the reference of tests/stem_ref.py against torch.nn.functional.conv2d(stride 2, pad 3) and autograd in float64, and its im2col rows against
    torch's unfold and against the conv they stand for (rows x weights = the conv)
  * exactness: for every exact case the float32 and the float64 evaluation agree bit for bit, and each channel's sum |y| and sum y^2, counted
    in units of the products' granularity, stay below 2^24 -- so the slab sums are exact in any order; every tap has a weight somewhere
  * the normalisation formula is the one the launchers compute: (raw - mean) * (1 / std), not a division and not a fused multiply-add
  * octseg_stem_op refuses, before any launch, what the launchers cannot take (nothing is launched: no GPU needed)
  * the wrappers' extent arithmetic
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

import conv_ref as CR
import stem_cases as SC
import stem_ref as SR
import sweep_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import convops as CO
from oct_segmentation_amd.convops import Stem


def reference(case, t):
    if case.stage == SC.FWD:
        return SR.forward(case.stem, t, case.T)
    if case.stage == SC.WGRAD:
        return SR.backward_weight(case.stem, t, case.T)
    return {'col': SR.im2col(case.stem, t, case.T)}


def test_case_ids_are_unique_and_the_table_is_whole():
    ids = [c.id for c in SC.all_cases()]
    assert len(set(ids)) == len(ids)
    for T in (SC.BF16, SC.F16):
        names = {c.name for c in SC.forward_cases(T)}
        assert {'ragged', 'tiny', 'persistent', 'eval', 'gauss'} <= names
    assert {c.name for c in SC.wgrad_cases()} >= {'ragged', 'tiny', 'persistent', 'gauss'}
    assert len(SC.im2col_cases()) == 3 * 3 * 2
    # the geometry the shapes are chosen for: 4 x 32-pixel tiles, at most 512 workgroups = slab rows
    tiles = lambda n, h, w: n * ((h // 2 + 3) // 4) * ((w // 2 + 31) // 32)
    assert tiles(*SC.RAGGED) == 2 * 5 * 2 and CO.stem_slab_rows(Stem(*SC.RAGGED)) == 20
    assert tiles(*SC.TINY) == 1 and CO.stem_slab_rows(Stem(*SC.TINY)) == 1
    assert tiles(*SC.PERSISTENT) == 525 and CO.stem_slab_rows(Stem(*SC.PERSISTENT)) == 512
    assert L.lib().octseg_stem_slab_rows(0, 8, 8) == 0


@pytest.mark.parametrize('case', [c for c in SC.all_cases() if c.exact and c.stage != SC.IM2COL], ids=lambda c: c.id)
def test_exact_cases_are_exact(case):
    t = SC.make_operands(case)
    r64 = reference(case, t)
    with R.as_float32():
        r32 = reference(case, t)
    for k in r64:
        assert r32[k].dtype == torch.float32 and r64[k].dtype == torch.float64
        assert torch.equal(r32[k].to(torch.float64), r64[k]), f'{case.id} {k}: the float32 and float64 references differ'
    if case.stage == SC.FWD:
        w = SR.weight_as_seen(t, case.T)
        assert bool((w != 0).any(dim=0).all()), f'{case.id}: a tap without a weight in any output channel'
        g = CR.lowbit(w) * CR.lowbit(SR.frame_as_seen(case.stem, t, case.T))
        y = r64['yf']
        s1 = float(y.abs().sum(dim=(0, 2, 3)).max()) / g
        s2 = float((y * y).sum(dim=(0, 2, 3)).max()) / (g * g)
        print(f'{case.id}: granularity {g}, max channel sum|y| = {s1:.0f} units, sum y^2 = {s2:.0f} units^2')
        if 'slab' in case.has:
            assert s1 < 2 ** 24 and s2 < 2 ** 24, f'{case.id}: channel sums leave float32 ({s1:.3g}, {s2:.3g} units): thin the weights'
        # one output: at most 147 products of at most 4 x 1 (x |wscale| <= 1) + |bias| <= 3, in sixteenths
        assert float(y.abs().max()) / g < 2 ** 24 and float(y.abs().max()) <= 147 * 4 + 3
    else:
        mag = CR.ref(t['dW']).abs() + SR.backward_weight_terms(case.stem, t, case.T, absolute=True)
        assert float(mag.max()) < 2 ** 24, f'{case.id}: a weight-gradient sum leaves float32'        # integers: the unit is 1
        assert torch.equal(r64['dW'][:, 147:], CR.ref(t['dW'])[:, 147:])                                # the padding columns keep what they held


def test_reference_matches_torch_functional_and_autograd():
    for case in [c for c in SC.forward_cases(SC.BF16) if c.name in ('ragged', 'tiny', 'eval', 'gauss')]:
        st = case.stem
        t = SC.make_operands(case)
        x = SR.frame_as_seen(st, t, case.T).clone().requires_grad_(True)
        w = SR.weight_as_seen(t, case.T).clone().requires_grad_(True)
        y = F.conv2d(x, w, stride=2, padding=3)
        assert y.shape[2:] == st.out_hw
        # the im2col rows times the weight matrix are that conv (an independent path: indexing against torch's own padding and striding)
        col = SR.im2col(st, t, case.T)
        wk = w.detach().permute(0, 2, 3, 1).reshape(64, 147)
        y_rows = torch.einsum('nyxk,ok->noyx', col[..., :147], wk)
        assert bool((col[..., 147:] == 0).all())
        assert float((y_rows - y.detach()).abs().max()) <= 1e-12 * float(y.detach().abs().max())
        full = y.detach()
        if t.get('bias') is not None:
            full = full + t['bias'].double().view(1, -1, 1, 1)
        if st.relu_out:
            full = full.clamp_min(0)
        assert torch.equal(full, SR.forward_f32value(st, t, case.T)), case.id
        # weight gradient: autograd of the same conv, laid out as [64][160]
        tw = SC.make_operands(SC.Case(case.name, SC.WGRAD, SC.BF16, st, exact=case.exact))
        tw['img'] = t['img']
        dy = CR.nchw(CR.ref(tw['dy']))
        gw, = torch.autograd.grad(y, (w,), dy)
        want = gw.permute(0, 2, 3, 1).reshape(64, 147)
        got = SR.backward_weight_terms(st, tw, SC.BF16)
        assert float((got[:, :147] - want).abs().max()) <= 1e-12 * float(want.abs().max()) and bool((got[:, 147:] == 0).all()), case.id


@pytest.mark.parametrize('k,p,KP', CO.STEM_KINDS)
def test_im2col_reference_matches_unfold(k, p, KP):
    """torch's unfold over the frame padded as the stem convs pad it (top / left p; bottom / right what a H / 2 output needs): channel order (c, r, s)."""
    st = Stem(2, 12, 20, ksize=k, pad=p, KP=KP, **SC.IMAGENET)
    t = SC.make_operands(SC.Case('u', SC.IM2COL, SC.BF16, st))
    x = SR.frame_as_seen(st, t, SC.BF16)
    oh, ow = st.out_hw
    xp = F.pad(x, (p, k - 2 - p, p, k - 2 - p))
    u = F.unfold(xp, kernel_size=k, stride=2)
    assert u.shape == (2, 3 * k * k, oh * ow)
    u = u.view(2, 3, k, k, oh, ow).permute(0, 4, 5, 2, 3, 1).reshape(2, oh, ow, 3 * k * k)
    col = SR.im2col(st, t, SC.BF16)
    assert torch.equal(col[..., :3 * k * k], u) and bool((col[..., 3 * k * k:] == 0).all())


def test_normalisation_formula_is_subtract_then_multiply_by_the_reciprocal():
    """(raw - mean) * (1 / std) in float32 differs from (raw - mean) / std and from the float64 value on a visible share of a uniform frame:
    a reference that used either would not be bit-exact.  The reference evaluates the same formula in both reference dtypes."""
    st = Stem(2, 12, 20, **SC.IMAGENET)
    t = SC.make_operands(SC.Case('n', SC.IM2COL, SC.F32, st))
    seen = SR.frame_as_seen(st, t, SC.F32)
    with R.as_float32():
        assert torch.equal(SR.frame_as_seen(st, t, SC.F32).double(), seen)
    x = t['img']
    mean, std = torch.tensor(st.mean).view(1, 3, 1, 1), torch.tensor(st.std).view(1, 3, 1, 1)
    assert int((((x - mean) / std).double() != seen).sum()) > 50
    assert int((((x.double() - mean.double()) / std.double()) != seen).sum()) > 50
    m = torch.tensor(st.mean, dtype=torch.float32)
    i = torch.ones(3) / torch.tensor(st.std, dtype=torch.float32)
    v = float(x[1, 2, 3, 4])
    assert float(seen[1, 2, 3, 4]) == float((torch.tensor(v) - m[2]) * i[2])
    # without normalize the frame passes untouched whatever mean / std say
    raw = Stem(2, 12, 20, mean=(1.0, 2.0, 3.0), std=(4.0, 5.0, 6.0))
    assert torch.equal(SR.frame_as_seen(raw, t, SC.F32), x.double())


# ------------------------------------------------------------------------------------------------ refusals (nothing is launched: no GPU needed)
def fake_ptrs(stage, has=()):
    return {k: 0x10000 * (i + 1) for i, k in enumerate(CO.stem_operand_names(stage, has))}


def _rc(stage, dt, stem, ptrs):
    """A refused call returns before anything touches the GPU; an accepted one would launch, so only refusals are asked for here."""
    return L.lib().octseg_stem_op(stage, dt, C.byref(CO.make_stem_desc(stem, ptrs)), None)


def test_entry_refuses_what_the_launchers_cannot_take():
    BAD_SHAPE, BAD_DTYPE, BAD_ARG = -1, -2, -5
    ok = Stem(2, 36, 88)
    fwd, wg, col = fake_ptrs(SC.FWD), fake_ptrs(SC.WGRAD), fake_ptrs(SC.IM2COL)
    # dtypes
    assert _rc(SC.FWD, L.F32, ok, fwd) == BAD_DTYPE and _rc(SC.WGRAD, L.F32, ok, wg) == BAD_DTYPE and _rc(SC.WGRAD, L.F16, ok, wg) == BAD_DTYPE
    assert _rc(SC.FWD, 3, ok, fwd) == BAD_DTYPE and _rc(3, L.BF16, ok, fwd) == BAD_ARG
    assert L.lib().octseg_stem_op(SC.FWD, L.BF16, None, None) == BAD_ARG
    # extents: the kernels compute H / 2
    for stage, p in ((SC.FWD, fwd), (SC.WGRAD, wg), (SC.IM2COL, col)):
        for bad in (Stem(2, 35, 88), Stem(2, 36, 87), Stem(0, 36, 88), Stem(1, 0, 8), Stem(1, 8, 1), Stem(16384, 512, 512)):
            assert _rc(stage, L.BF16, bad, p) == BAD_SHAPE, (stage, bad)
        assert 'stem_op' in L.lib().octseg_last_error().decode()
    # pointers
    for stage, p in ((SC.FWD, fake_ptrs(SC.FWD, ('wscale', 'bias', 'slab'))), (SC.WGRAD, wg), (SC.IM2COL, col)):
        for k in p:
            q = dict(p); q[k] += 8
            assert _rc(stage, L.BF16, ok, q) == BAD_ARG, (stage, k)
        for k in CO.stem_operand_names(stage):
            q = dict(p); del q[k]
            assert _rc(stage, L.BF16, ok, q) == BAD_ARG, (stage, k)
    # the fused fields
    ro = Stem(2, 36, 88, relu_out=True)
    assert _rc(SC.FWD, L.BF16, ro, fwd) == BAD_ARG                                                    # relu_out without bias
    assert _rc(SC.FWD, L.F16, ro, fake_ptrs(SC.FWD, ('bias', 'slab'))) == BAD_ARG                     # relu_out with the slab
    assert _rc(SC.FWD, L.BF16, Stem(2, 36, 88, slab_row0=-1), fake_ptrs(SC.FWD, ('slab',))) == BAD_ARG
    assert _rc(SC.FWD, L.BF16, ok, {**fwd, 'dW': 0x900000}) == BAD_ARG and _rc(SC.FWD, L.BF16, ok, {**fwd, 'dy': 0x900000}) == BAD_ARG
    for k in ('w', 'wscale', 'bias', 'y', 'slab'):
        assert _rc(SC.WGRAD, L.BF16, ok, {**wg, k: 0x900000}) == BAD_ARG, k                            # forward-only fields
    assert _rc(SC.WGRAD, L.BF16, ro, wg) == BAD_ARG and _rc(SC.WGRAD, L.BF16, Stem(2, 36, 88, slab_row0=1), wg) == BAD_ARG
    # normalisation
    assert _rc(SC.FWD, L.BF16, Stem(2, 36, 88, normalize=True, std=(0.2, 0.0, 0.2)), fwd) == BAD_ARG
    assert _rc(SC.IM2COL, L.F32, Stem(2, 36, 88, normalize=True, std=(0.2, -1.0, 0.2)), col) == BAD_ARG
    assert _rc(SC.IM2COL, L.F32, Stem(2, 36, 88, normalize=True, mean=(float('nan'), 0, 0)), col) == BAD_ARG
    d = CO.make_stem_desc(ok, fwd); d.normalize = 2
    assert L.lib().octseg_stem_op(SC.FWD, L.BF16, C.byref(d), None) == BAD_ARG
    # im2col kinds: the three the builders use
    for k, p, KP in ((7, 3, 32), (7, 2, 160), (5, 2, 160), (3, 1, 160), (3, 2, 32), (3, 1, 28)):
        assert _rc(SC.IM2COL, L.BF16, Stem(2, 36, 88, ksize=k, pad=p, KP=KP), col) == BAD_SHAPE, (k, p, KP)
    # the deterministic-reduction mode takes the weight gradient off this kernel (plan_backward.cpp): refused, not rerouted
    import os
    before = 1 if os.environ.get('OCTSEG_DETERMINISTIC') is not None else 0
    L.check(L.lib().octseg_set_deterministic(1))
    try:
        assert _rc(SC.WGRAD, L.BF16, ok, wg) == BAD_ARG
        assert 'deterministic' in L.lib().octseg_last_error().decode()
    finally:
        L.check(L.lib().octseg_set_deterministic(before))


def test_wrappers_derive_every_extent_from_the_frame():
    st = Stem(3, 198, 432)
    assert st.img_shape == (3, 3, 198, 432) and st.out_hw == (99, 216)
    assert st.y_shape == (3, 99, 216, 64) and st.col_shape == (3, 99, 216, 160) and st.w_shape == (64, 160)
    assert Stem(2, 12, 20, ksize=3, pad=0, KP=32).col_shape == (2, 6, 10, 32)
    assert CO.stem_operand_names(SC.FWD, ('bias', 'slab')) == ['img', 'w', 'y', 'bias', 'slab']
    d = CO.make_stem_desc(Stem(2, 36, 88, relu_out=True, slab_row0=3, **SC.IMAGENET), {'img': 0x1000, 'y': 0x2000, 'slab': 0x3000})
    assert (d.N, d.H, d.W, d.normalize, d.relu_out, d.slab_row0, d.ksize, d.pad, d.KP) == (2, 36, 88, 1, 1, 3, 7, 3, 160)
    assert (d.img, d.y, d.stat_slab, d.w, d.dy, d.dW, d.col) == (0x1000, 0x2000, 0x3000, None, None, None, None)
    assert abs(d.mean[1] - 0.456) < 1e-7 and abs(d.stdv[2] - 0.225) < 1e-7

    class FakeTensor:       # what check_stem_tensors looks at, without a device
        def __init__(self, shape, dtype):
            self.shape, self.dtype, self.is_cuda = torch.Size(shape), dtype, True

        def is_contiguous(self):
            return True

        def dim(self):
            return len(self.shape)

    small = Stem(2, 36, 88, slab_row0=3)
    good = {'img': FakeTensor(small.img_shape, SC.F32), 'w': FakeTensor((64, 160), SC.F32), 'y': FakeTensor(small.y_shape, SC.BF16),
            'slab': FakeTensor((3 + 20, 64, 2), SC.F32)}
    CO.check_stem_tensors(SC.FWD, small, good, SC.BF16)
    for k, v in (('y', FakeTensor((2, 18, 44, 32), SC.BF16)), ('y', FakeTensor(small.y_shape, SC.F16)), ('w', FakeTensor((64, 147), SC.F32)),
                 ('img', FakeTensor((2, 3, 36, 80), SC.F32)), ('slab', FakeTensor((3 + 19, 64, 2), SC.F32)), ('slab', FakeTensor((23, 32, 2), SC.F32))):
        with pytest.raises(AssertionError):
            CO.check_stem_tensors(SC.FWD, small, {**good, k: v}, SC.BF16)
    with pytest.raises(AssertionError):
        CO.check_stem_tensors(SC.FWD, small, {**good, 'dW': FakeTensor((64, 160), SC.F32)}, SC.BF16)       # a tensor the stage does not take
    with pytest.raises(AssertionError):
        CO.check_stem_tensors(SC.WGRAD, small, {'img': good['img'], 'dy': FakeTensor(small.y_shape, SC.BF16), 'dW': FakeTensor((64, 147), SC.F32)}, SC.BF16)
