"""Single-launch parity of the conv kernels' fused operand and epilogue paths against the float64 reference of tests/conv_ref.py.

One layer pass per call through octseg_conv_layer_op (oct_segmentation_amd/convops.py) with the descriptors the plan builds: lazy
BatchNorm affine + ReLU per source, nearest-x2 reads, concatenation on and off the K chunk, the eval fold (wscale, bias, relu_out), the
BatchNorm statistics slab (slab_row0 > 0 included), several data-gradient destinations with accum and pool, the head's NCHW f32 store.
The cases and how each is judged are listed in tests/conv_cases.py (exact operands: equality with the reference rounded by the route's store
rule; Gaussian operands: Rule R of sweep_ref.py); tests/test_convops.py proves on the CPU that the exact cases are exact.  The route of
every launch is asserted through octseg_conv_layer_route on the very pointers that are launched.

Buffers: every destination, slab and dW is an interior view of an allocation with 4 KiB NaN margins and starts as NaN where the launch
stores, as known values where it accumulates; inputs sit between margins of a large finite poison.  After a group's single synchronise every
margin must be untouched, every owned element finite, and the slab rows outside [slab_row0, slab_row0 + rows) still NaN.

Routes: conv_mfma's 16-pixel tilings (f32, bf16) and 11 x 11 tiles, gemm1x1, conv3x3p, thin.hip (3x3, 1x1, ConvTranspose2d parities, head),
and the weight gradients of wgrad_mfma (1, 4, 9 taps), thin.hip, wgrad1x1 and wgrad_convt, in split-K and in deterministic mode.
The eval-fold cases pin the bias / relu_out epilogue of every route; the fold arithmetic itself (W * wscale in f32, then rounded) is thin.hip's own
on the thin route and the single-op packer's (launch_pack_weight_image) on the image-consuming routes -- plans fold in pack_all_kernel.
'mfma-16' names every 16-pixel-wide loop of conv_mfma_kernel (generic, resident, 1x1, the run9 / run9s slab rings, the four-tap masked loop of
a wide ConvTranspose2d parity: the convT_wide case); which of the rings a case runs is choose()'s business and is not asserted.
NOT covered: conv_mfma's wide-N tile (256 -> 256 on >= 1024 workgroups: its CPU reference takes tens of seconds; tests/test_gpu_ops.py and the
whole-network tests keep it).  The tied K4 images and per-source tap subsets have tests/test_gpu_tiedops.py (one pass at a time; whole networks:
tests/test_gpu_tied.py), the 7x7 stem kernels and the stem im2col tests/test_gpu_stemops.py.
"""
import copy
import ctypes as C
import os

import pytest
import torch

import conv_cases as CC
import conv_ref as CR
import sweep_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import convops as CO

pytestmark = pytest.mark.gpu

INPUTS = ('x', 'dy')        # operands that sit between poison margins (the tensors whose halo a kernel might read)


def stage(case, G):
    """The case's operands on the device, guarded; returns (cpu operands, device operands)."""
    t = CC.make_operands(case)
    dev = {}
    for k, v in t.items():
        dev[k] = G.put_poisoned(v) if k.startswith(INPUTS) else G.put(v)
    return t, dev


def launch(case, dev):
    ptrs = {k: v.data_ptr() for k, v in dev.items()}
    got = CO.route(case.mode, case.dt, case.layer, ptrs)
    assert tuple(got) == tuple(case.route), f'route {got}, the case names {case.route}'
    CO.conv_layer(case.mode, case.layer, dev)


def where(shape, i, head=False):
    idx = []
    for s in reversed(shape):
        idx.append(i % s)
        i //= s
    idx.reverse()
    names = ('n', 'channel', 'y', 'x') if head else (('n', 'y', 'x', 'channel') if len(shape) == 4 else ('row', 'channel', 'k'))
    return ', '.join(f'{n} {v}' for n, v in zip(names, idx))


def expect_equal(got, want, what, names=None):
    """Numeric equality of every element (a NaN -- an element nobody wrote -- is unequal to everything; the sign of a zero is not compared)."""
    g = got.detach().cpu().to(torch.float64)
    w = want.reshape(g.shape).to(torch.float64)
    assert bool(torch.isfinite(g).all()), f'{what}: {int((~torch.isfinite(g)).sum())} of {g.numel()} owned elements are not finite'
    bad = (g != w).reshape(-1).nonzero().reshape(-1)
    if bad.numel():
        i = int(bad[0])
        raise AssertionError(f'{what}: {bad.numel()} of {g.numel()} elements differ; first at {names(tuple(g.shape), i) if names else i}: '
                             f'expected {w.reshape(-1)[i].item()!r}, got {g.reshape(-1)[i].item()!r}')


def check_slab(case, t, dev, ref_stats):
    Ly = case.layer
    rows = CO.slab_rows(case.dt, Ly, {k: v.data_ptr() for k, v in dev.items()}, has=case.has)
    slab = dev['slab'].cpu()
    assert slab.shape[0] == Ly.slab_row0 + rows + CC.SLAB_TAIL
    keep = torch.ones(slab.shape[0], dtype=torch.bool)
    keep[Ly.slab_row0:Ly.slab_row0 + rows] = False
    assert torch.equal(R.bits_of(slab[keep]), R.bits_of(t['slab'][keep])), f'{case.id}: a slab row outside [{Ly.slab_row0}, {Ly.slab_row0 + rows}) was written'
    own = slab[Ly.slab_row0:Ly.slab_row0 + rows].to(torch.float64)
    assert bool(torch.isfinite(own).all()), f'{case.id}: {int((~torch.isfinite(own)).sum())} slab values of the launch\'s own rows were never written'
    expect_equal(own.sum(dim=0), ref_stats, f'{case.id} slab (sum over its {rows} rows of sum y, sum y^2)', lambda s, i: f'channel {i // 2}, {"sum y^2" if i % 2 else "sum y"}')


def check_exact(case, t, dev):
    Ly = case.layer
    if case.mode == CC.FWD:
        r = CR.forward(Ly, t, case.T, case.rule)
        expect_equal(dev['y'], r['y'], f'{case.id} y', lambda s, i: where(s, i, Ly.head))
        if 'slab' in case.has:
            check_slab(case, t, dev, r['stats'])
    elif case.mode == CC.DGRAD:
        r = CR.backward_data(Ly, t, case.T, case.rule)
        for i in range(len(Ly.srcs)):
            expect_equal(dev[f'dx{i}'], r[f'dx{i}'], f'{case.id} dx{i}', where)
    else:
        expect_equal(dev['dW'], CR.backward_weight(Ly, t, case.T)['dW'], f'{case.id} dW', lambda s, i: 'tap (%d, %d), co %d, ci %d' % (
            i // (s[1] * s[2] * s[3]), i // (s[2] * s[3]) % s[1], i // s[3] % s[2], i % s[3]))


def check_rounding(case, t, dev):
    """Rule R: |got - ref| <= n eps32 sum|terms| (+ half an ulp of T where the result is stored as T); n = the terms added per output."""
    Ly, T = case.layer, case.T
    if case.mode == CC.FWD:
        ref = CR.forward_f32value(Ly, t, T)
        mag = CR.conv_of(Ly, CR.virtual_input(Ly, t, T).abs(), CR.weight_as_seen(Ly, t, T).abs())
        n = Ly.R * Ly.R * Ly.Cin
        if t.get('bias') is not None:
            mag, n = mag + CR.ref(t['bias']).abs().view(1, -1, 1, 1), n + 1
        R.assert_within(dev['y'], CR.nhwc(ref), CR.nhwc(R.bound_r(ref, mag, n, T)), f'{case.id} y')
    else:
        oh, ow = Ly.out_hw
        n = Ly.N * oh * ow + 1
        ref = CR.backward_weight(Ly, t, T)['dW']
        mag = CR.ref(t['dW']).abs() + CR.backward_weight_terms(Ly, t, T, absolute=True)
        R.assert_within(dev['dW'], ref, R.bound_r(ref, mag, n), f'{case.id} dW')


def run_group(cases, dev):
    """Launch every case, synchronise once, then judge every case (a failure does not hide the ones behind it)."""
    G = CR.Guard(dev)
    staged, failures = [], []
    for case in cases:
        try:
            t, d = stage(case, G)
            launch(case, d)
            staged.append((case, t, d))
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
    for case, t, d in staged:
        try:
            (check_exact if case.exact else check_rounding)(case, t, d)
        except AssertionError as e:
            failures.append(f'{case.id}: {str(e)[:600]}')
    assert not failures, f'{len(failures)} failures in {len(cases)} cases:\n' + '\n'.join(failures)


@pytest.mark.parametrize('group,T', CC.GROUP_PARAMS, ids=CC.GROUP_IDS)
def test_conv_route(group, T, cuda):
    run_group(CC.group_cases(group, T), cuda)


def test_weight_gradients_in_deterministic_mode(cuda):
    """The exact weight-gradient cases again without split-K (one writer per dW element): the same sums, bit for bit.  thin.hip's weight
    gradient steps aside in this mode (thin_wgrad_eligible), so those cases run through wgrad_mfma here."""
    cases = CC.group_cases('wgrad', CC.BF16) + CC.group_cases('wgrad', CC.F32)
    for c in cases:
        c.route = tuple('mfma' if r == 'thin' else r for r in c.route)
    before = 1 if os.environ.get('OCTSEG_DETERMINISTIC') is not None else 0      # the mode a process starts in (deterministic_mode(), api.cpp); no test leaves another
    L.check(L.lib().octseg_set_deterministic(1))
    try:
        run_group(cases, cuda)
    finally:
        L.check(L.lib().octseg_set_deterministic(before))


def test_refused_calls_write_nothing(cuda):
    """Well-formed device buffers, ill-formed descriptors: refused before any launch, and every buffer still holds what it held."""
    case = CC.group_cases('mfma16', CC.BF16)[0]
    G = CR.Guard(cuda)
    t, dev = stage(case, G)
    before = {k: v.clone() for k, v in dev.items()}
    ptrs = {k: v.data_ptr() for k, v in dev.items()}
    ptrs['scratch'] = G.empty((CO.scratch_bytes(case.layer, case.dt),), torch.uint8).data_ptr()
    lib = L.lib()

    def op(mode, dt, layer, p, nbytes=1 << 30):
        return lib.octseg_conv_layer_op(mode, dt, C.byref(CO.make_desc(layer, p, nbytes)), L.stream_ptr())
    ro = copy.deepcopy(case.layer); ro.relu_out = True                 # relu_out with the slab
    assert op(CC.FWD, case.dt, ro, {**ptrs, 'bias': ptrs['shift0']}) == -5
    assert op(CC.FWD, case.dt, case.layer, {**ptrs, 'y': ptrs['y'] + 2}) == -5
    assert op(CC.FWD, case.dt, case.layer, {k: v for k, v in ptrs.items() if k != 'shift0'}) == -5
    assert op(CC.FWD, case.dt, case.layer, ptrs, nbytes=16) == -5
    assert op(CC.DGRAD, L.F16, case.layer, ptrs) == -2
    pl = copy.deepcopy(case.layer); pl.pool = (1, 0, 0, 0, 0)
    assert op(CC.FWD, case.dt, pl, ptrs) == -5
    torch.cuda.synchronize()
    G.check()
    for k, v in dev.items():
        assert torch.equal(R.bits_of(v) if v.dtype.is_floating_point else v, R.bits_of(before[k]) if v.dtype.is_floating_point else before[k]), k
