"""Single-launch parity of the stem kernels against the float64 reference of tests/stem_ref.py.

One launch per call through octseg_stem_op (oct_segmentation_amd/convops.py: stem()): thin.hip's KSTEM forward (training: the BatchNorm
statistics slab, slab_row0 > 0 included; eval: wscale, bias, relu_out folded in thin.hip) in bf16 and f16, its weight gradient in bf16, and
launch_stem_im2col with the three (ksize, pad) pairs of the builders in f32, bf16 and f16.  The cases and how each is judged are listed in
tests/stem_cases.py (exact operands: equality with the reference rounded by the store rule; Gaussian operands: Rule R of sweep_ref.py; im2col: bit
for bit); tests/test_stemops.py proves on the CPU that the exact cases are exact.  The path f32 and the deterministic mode take -- the im2col
rows followed by a 1x1 layer of 160 input channels through octseg_conv_layer_op -- is pinned against the same stem reference.

Buffers: as in tests/test_gpu_convops.py.  y, col, slab and dW are interior views of allocations with 4 KiB NaN margins and start as NaN where
the launch stores, as known integers where it accumulates (dW); the frame and dy sit between margins of a large finite poison.  After a group's
single synchronise every margin must be untouched, every owned element finite, the slab rows outside [slab_row0, slab_row0 + rows) still
NaN, the weight columns 147..159 of dW what they were.  Every forward and im2col case is launched a second time into fresh buffers: bit for bit
the same (the weight gradient ends in float atomics: its exact cases are order-free by construction instead).

Measured on an MI355X: see MEASURED below.
"""
import copy
import ctypes as C
import os

import pytest
import torch

import conv_ref as CR
import stem_cases as SC
import stem_ref as SR
import sweep_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import convops as CO
from oct_segmentation_amd.convops import Layer, Src
from test_gpu_convops import expect_equal, where

pytestmark = pytest.mark.gpu

MEASURED = """
Largest |got - ref| / Rule R bound of the Gaussian cases ("RATIO" lines of the run; 1 = at the bound):
  forward, eval fold (wscale, bias, relu_out)   bf16 0.979   f16 0.963        forward, plain store   bf16 0.981   f16 0.939
  (near 1: half a unit in the last place of T is the bound's first term, and some element always rounds by nearly that much)
  weight gradient   bf16 below 0.0005 (n = N OH OW + 1 = 1585 terms: the bound is generous, as for the conv weight gradients)
Every exact case, slab, im2col case and both compositions: equal bit for bit.  Before stem_im2col_kernel kept its product in f32, the case
k3p1_norm f16 differed on 2 of 3840 elements by one f16 ulp (0.449951171875 against 0.4501953125).
The file runs in 1.4 s (its slowest test, the bf16 forwards with the 3 x 198 x 432 frame: 0.4 s).
"""

INPUTS = ('img', 'dy')      # operands that sit between poison margins
OUTPUTS = {SC.IM2COL: ('col',), SC.FWD: ('y', 'slab'), SC.WGRAD: ()}


def stage_case(case, G):
    t = SC.make_operands(case)
    dev = {k: (G.put_poisoned(v) if k in INPUTS else G.put(v)) for k, v in t.items()}
    again = dict(dev)       # the second launch: the same inputs, fresh destinations
    for k in OUTPUTS[case.stage]:
        if k in t:
            again[k] = G.put(t[k])
    return t, dev, again


def w_where(shape, i):
    return f'co {i // shape[1]}, k {i % shape[1]} (tap ({i % shape[1] // 21}, {i % shape[1] % 21 // 3}), channel {i % 3})'


def share(got, ref, bound):
    """Largest |got - ref| / bound over the tensor (1 = at the bound)."""
    err = (R.d(got).reshape(ref.shape) - ref).abs()
    return float((err / bound).max())


def check_slab(case, t, dev, ref_stats):
    st = case.stem
    rows = CO.stem_slab_rows(st)
    slab = dev['slab'].cpu()
    assert slab.shape[0] == st.slab_row0 + rows + SC.SLAB_TAIL
    keep = torch.ones(slab.shape[0], dtype=torch.bool)
    keep[st.slab_row0:st.slab_row0 + rows] = False
    assert torch.equal(R.bits_of(slab[keep]), R.bits_of(t['slab'][keep])), f'{case.id}: a slab row outside [{st.slab_row0}, {st.slab_row0 + rows}) was written'
    own = slab[st.slab_row0:st.slab_row0 + rows].to(torch.float64)
    assert bool(torch.isfinite(own).all()), f'{case.id}: {int((~torch.isfinite(own)).sum())} slab values of the launch\'s own rows were never written'
    expect_equal(own.sum(dim=0), ref_stats, f'{case.id} slab (sum over its {rows} rows of sum y, sum y^2)', lambda s, i: f'channel {i // 2}, {"sum y^2" if i % 2 else "sum y"}')


def check(case, t, dev):
    st, T = case.stem, case.T
    if case.stage == SC.IM2COL:
        R.assert_exact(dev['col'], SR.im2col(st, t, T), f'{case.id} col')
    elif case.stage == SC.FWD and case.exact:
        r = SR.forward(st, t, T)
        expect_equal(dev['y'], r['y'], f'{case.id} y', where)
        if 'slab' in case.has:
            check_slab(case, t, dev, r['stats'])
    elif case.stage == SC.FWD:
        ref = SR.forward_f32value(st, t, T)
        mag = torch.nn.functional.conv2d(SR.frame_as_seen(st, t, T).abs(), SR.weight_as_seen(t, T).abs(), stride=2, padding=3)
        n = SR.KTAPS
        if t.get('bias') is not None:
            mag, n = mag + CR.ref(t['bias']).abs().view(1, -1, 1, 1), n + 1
        bound = CR.nhwc(R.bound_r(ref, mag, n, T))
        R.assert_within(dev['y'], CR.nhwc(ref), bound, f'{case.id} y')
        print(f'RATIO {case.id} {share(dev["y"], CR.nhwc(ref), bound):.3f}')
    else:
        ref = SR.backward_weight(st, t, T)['dW']
        if case.exact:
            expect_equal(dev['dW'], ref, f'{case.id} dW', w_where)
        else:
            oh, ow = st.out_hw
            mag = CR.ref(t['dW']).abs() + SR.backward_weight_terms(st, t, T, absolute=True)
            bound = R.bound_r(ref, mag, st.N * oh * ow + 1)
            # (the padding columns hold integers and receive +0: a zero bound, met with equality)
            R.assert_within(dev['dW'], ref, bound, f'{case.id} dW')
            print(f'RATIO {case.id} {share(dev["dW"][:, :147], ref[:, :147], bound[:, :147]):.3f}')
        got = dev['dW'].cpu()
        assert torch.equal(R.bits_of(got[:, 147:].contiguous()), R.bits_of(t['dW'][:, 147:].contiguous())), f'{case.id}: weight columns 147..159 changed'


def run_group(cases, dev):
    """Launch every case (the stores twice), synchronise once, then judge every case (a failure does not hide the ones behind it)."""
    G = CR.Guard(dev)
    staged, failures = [], []
    for case in cases:
        try:
            t, d, again = stage_case(case, G)
            CO.stem(case.stage, case.stem, d)
            if OUTPUTS[case.stage]:
                CO.stem(case.stage, case.stem, again)
            staged.append((case, t, d, again))
        except AssertionError as e:
            failures.append(f'{case.id}: {str(e)[:400]}')
        except RuntimeError as e:
            if 'HIP' in str(e) or 'octseg error -4' in str(e):      # a HIP error: nothing more is started on this GPU
                pytest.exit(f'{case.id}: {e!r}', returncode=3)
            failures.append(f'{case.id}: {e!r}'[:400])
    torch.cuda.synchronize()
    try:
        G.check()
    except AssertionError as e:
        failures.append(f'guards: {e}')
    for case, t, d, again in staged:
        try:
            check(case, t, d)
            for k in OUTPUTS[case.stage]:
                if k in t:
                    assert torch.equal(R.bits_of(d[k]), R.bits_of(again[k])), f'{case.id}: a second launch wrote another {k}'
        except AssertionError as e:
            failures.append(f'{case.id}: {str(e)[:600]}')
    assert not failures, f'{len(failures)} failures in {len(cases)} cases:\n' + '\n'.join(failures)


@pytest.mark.parametrize('T', [SC.BF16, SC.F16], ids=['bf16', 'f16'])
def test_stem_forward(T, cuda):
    run_group(SC.forward_cases(T), cuda)


def test_stem_weight_gradient(cuda):
    run_group(SC.wgrad_cases(), cuda)


def test_stem_im2col(cuda):
    run_group(SC.im2col_cases(), cuda)


def _composed(T, cuda, G, wgrad):
    """IM2COL into a guarded col tensor, then the 1x1 layer over it; returns (cpu operands, device tensors, stem)."""
    st = CO.Stem(*SC.RAGGED)
    oh, ow = st.out_hw
    t = SC.make_operands(SC.Case('composed', SC.WGRAD if wgrad else SC.FWD, T, st))
    layer = Layer(st.N, oh, ow, 1, 64, [Src(160)])
    img, col = G.put_poisoned(t['img']), G.empty(st.col_shape, T)
    CO.stem(SC.IM2COL, st, {'img': img, 'col': col})
    if wgrad:
        dev = {'x0': col, 'dy': G.put_poisoned(t['dy']), 'dW': G.put(t['dW'].view(1, 1, 64, 160))}
        mode = CO.BACKWARD_WEIGHT
    else:
        dev = {'x0': col, 'w': G.put(t['w'].view(1, 1, 64, 160)), 'y': G.empty(st.y_shape, T)}
        mode = CO.FORWARD
    routes = CO.route(mode, SC.DT[T], layer, {k: v.data_ptr() for k, v in dev.items()})
    CO.conv_layer(mode, layer, dev)
    return t, dev, st, routes


def test_im2col_then_1x1_is_the_stem_in_f32(cuda):
    """The f32 plan's stem: im2col rows + conv_mfma's 1x1 over KP = 160 (weight columns 147..159 meet zero rows).  Integer frames: equality."""
    G = CR.Guard(cuda)
    t, dev, st, routes = _composed(SC.F32, cuda, G, wgrad=False)
    torch.cuda.synchronize()
    G.check()
    assert routes == ['mfma-16'], routes
    expect_equal(dev['y'], SR.forward(st, t, SC.F32)['y'], 'composed f32 y', where)


def test_im2col_then_1x1_weight_gradient_in_deterministic_mode(cuda):
    """The deterministic mode's stem weight gradient: im2col rows rebuilt, then the atomics-free 1x1 weight gradient (plan_backward.cpp)."""
    before = 1 if os.environ.get('OCTSEG_DETERMINISTIC') is not None else 0
    L.check(L.lib().octseg_set_deterministic(1))
    try:
        G = CR.Guard(cuda)
        t, dev, st, routes = _composed(SC.BF16, cuda, G, wgrad=True)
        torch.cuda.synchronize()
        G.check()
    finally:
        L.check(L.lib().octseg_set_deterministic(before))
    ref = SR.backward_weight(st, t, SC.BF16)['dW']
    expect_equal(dev['dW'].view(64, 160), ref, f'composed deterministic dW ({routes})', w_where)


def test_refused_calls_write_nothing(cuda):
    """Well-formed device buffers, ill-formed descriptors: refused before any launch, and every buffer still holds what it held."""
    G = CR.Guard(cuda)
    fwd = SC.Case('refused', SC.FWD, SC.BF16, CO.Stem(*SC.RAGGED), ('bias', 'slab'))
    wg = SC.Case('refused', SC.WGRAD, SC.BF16, CO.Stem(*SC.RAGGED))
    (tf, df, _), (tw, dw, _) = stage_case(fwd, G), stage_case(wg, G)
    col = G.empty(fwd.stem.col_shape, torch.bfloat16)
    bufs = {**{f'f.{k}': v for k, v in df.items()}, **{f'w.{k}': v for k, v in dw.items()}, 'col': col}
    before = {k: v.clone() for k, v in bufs.items()}
    pf, pw = {k: v.data_ptr() for k, v in df.items()}, {k: v.data_ptr() for k, v in dw.items()}
    lib = L.lib()

    def op(stage, dt, stem, p):
        return lib.octseg_stem_op(stage, dt, C.byref(CO.make_stem_desc(stem, p)), L.stream_ptr())
    ro = copy.deepcopy(fwd.stem); ro.relu_out = True
    assert op(SC.FWD, L.BF16, ro, pf) == -5                                          # relu_out with the slab
    assert op(SC.FWD, L.BF16, ro, {k: v for k, v in pf.items() if k not in ('bias', 'slab')}) == -5
    assert op(SC.FWD, L.F32, fwd.stem, pf) == -2
    assert op(SC.FWD, L.BF16, fwd.stem, {**pf, 'y': pf['y'] + 2}) == -5
    assert op(SC.FWD, L.BF16, CO.Stem(2, 35, 88), pf) == -1
    assert op(SC.WGRAD, L.F16, wg.stem, pw) == -2
    assert op(SC.WGRAD, L.BF16, wg.stem, {**pw, 'y': pf['y']}) == -5
    assert op(SC.WGRAD, L.BF16, CO.Stem(2, 36, 90), {k: v for k, v in pw.items() if k != 'dW'}) == -5
    assert op(SC.IM2COL, L.BF16, CO.Stem(*SC.RAGGED, ksize=5, pad=2), {'img': pf['img'], 'col': col.data_ptr()}) == -1
    assert op(SC.IM2COL, L.BF16, CO.Stem(*SC.RAGGED), {'img': pf['img']}) == -5
    torch.cuda.synchronize()
    G.check()
    for k, v in bufs.items():
        assert torch.equal(R.bits_of(v), R.bits_of(before[k])), k
