"""Single-launch parity of the tied decoder layer against the float64 reference of the PLAIN layer (tests/tied_cases.py, tests/conv_ref.py).

One pass per call through octseg_tied_layer_op (oct_segmentation_amd/convops.py: tied_layer), which packs the 4x4 / masked / skip images with the
plan's own pack jobs (pack_all_kernel, PackJob::tied = 1 | 2 | 0 over a channel slice) and runs the launches tied_forward and the tied branches of
conv_backward run: the skip store + four accumulating parity launches; the masked launch over dy's parity planes (conv_mfma's LOOP_MASKED on the 8 x 16
tile and LOOP_MASKED_T11 on the 11 x 11 tile) or the 16-tap stride-2 launch, plus the skip slice's 3x3 data gradient with one destination per skip
source; wgrad_convt16 or four parity launches, the skip slice's weight gradient and launch_tied_fold onto a dW that already holds values, at
both split-K widths.  The route of every launch is asserted through octseg_tied_layer_route on the very pointers that are launched.

Judged as tests/test_gpu_convops.py judges: exact operands bit for bit against the reference rounded by the tied store rules (csrc/kernels.h),
Gaussian operands by Rule R; tests/test_tiedops.py proves on the CPU that the exact cases are exact and that the DENSE cases tell the tied rules from
the plain path's.  Buffers: destinations, dW and the scratch are interior views with 4 KiB NaN margins, NaN where a launch stores, known values
where it accumulates; sources and dy sit between poison margins; one synchronise per group; every margin untouched, every owned element finite.
Forward and data gradient are launched a second time into fresh destinations and a fresh scratch: bit for bit the same.

Measured on an MI355X: see MEASURED below.
"""
import copy
import ctypes as C
import os

import pytest
import torch

import conv_cases as CC
import conv_ref as CR
import sweep_ref as R
import tied_cases as TC
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import convops as CO
from test_gpu_convops import expect_equal, where

pytestmark = pytest.mark.gpu

MEASURED = """
Largest |got - ref| / Rule R bound of the Gaussian cases ("RATIO" lines of the run; 1 = at the bound):
  forward (Cs = 0)                   y 0.938
  data gradient, low resolution      m16_cs32 0.680   m11 0.448   u32 0.848        skip source   0.933   0.859   0.954
  (near 1: half a unit in the last place of bf16 is the bound's first term)
  weight gradient                    m16_cs32, m11 (both split-K widths) below 0.0005   u32 0.001   w1tile 0.010 (n = N H W + 1 terms: generous)
Every exact case (DENSE ones and deterministic mode included): equal bit for bit.  The file runs in 1.4 s (its slowest test: 0.25 s).
"""

INPUTS = ('x', 'dy')


def w_where(s, i):
    return 'tap (%d, %d), co %d, ci %d' % (i // (s[1] * s[2] * s[3]), i // (s[2] * s[3]) % s[1], i // s[3] % s[2], i % s[3])


def stage(tc, G):
    t = TC.make_operands(tc)
    dev = {k: (G.put_poisoned(v) if k.startswith(INPUTS) else G.put(v)) for k, v in t.items()}
    scratch = G.empty((CO.tied_scratch_bytes(tc.case.layer),), torch.uint8)
    again = None
    if tc.case.mode != CC.WGRAD:      # (the weight gradient ends in float atomics and a fold onto dW: its exact cases are order-free instead)
        again = dict(dev)
        for k in CC.OUTPUTS[tc.case.mode](tc.case.layer):
            again[k] = G.put(t[k])
        again = (again, G.empty((scratch.numel(),), torch.uint8))
    return t, dev, scratch, again


def launch(tc, dev, scratch, routes=None):
    c = tc.case
    ptrs = {k: v.data_ptr() for k, v in dev.items()}
    got = CO.tied_route(c.mode, c.layer, ptrs, wg_target=tc.wg_target)
    if routes is None:
        assert tuple(got) == tuple(c.route), f'route {got}, the case names {c.route}'
    else:
        assert set(got) <= routes, got
    CO.tied_layer(c.mode, c.layer, dev, wg_target=tc.wg_target, scratch=scratch)


def share(got, ref, bound):
    err = (R.d(got).reshape(ref.shape) - ref).abs()
    return float((err / bound).max())


def within(got, ref, bound, what):
    R.assert_within(got, ref, bound, what)
    print(f'RATIO {what} {share(got, ref, bound):.3f}')


def check_rounding(tc, t, dev):
    """Rule R against the plain layer: n = the products the plain layer adds per output, sum |terms| = the plain layer's (tied_cases docstring)."""
    c = tc.case
    Ly, T = c.layer, c.T
    Ca = Ly.srcs[0].C
    if c.mode == CC.FWD:
        assert len(Ly.srcs) == 1                   # (with skips the stored partials are rounded on the way: the exact cases carry that rule)
        ref, _ = TC.forward_parts(Ly, t, T)
        mag = CR.conv_of(Ly, CR.virtual_input(Ly, t, T).abs(), CR.weight_as_seen(Ly, t, T).abs())
        within(dev['y'], CR.nhwc(ref), CR.nhwc(R.bound_r(ref, mag, 9 * Ly.Cin, T)), f'{tc.id} y')
    elif c.mode == CC.DGRAD:
        assert not any(Ly.accum)
        low, full = TC.backward_data_values(Ly, t, T)
        ta = {'dy': t['dy'].abs(), 'w': t['w'].abs()}
        mlow, mfull = TC.backward_data_values(Ly, ta, T)
        within(dev['dx0'], CR.nhwc(low), CR.nhwc(R.bound_r(low, mlow, 36 * Ly.Cout, T)), f'{tc.id} dx0')
        c0 = Ca
        for i, s in enumerate(Ly.srcs[1:], start=1):
            ref, mag = full[:, c0:c0 + s.C], mfull[:, c0:c0 + s.C]
            within(dev[f'dx{i}'], CR.nhwc(ref), CR.nhwc(R.bound_r(ref, mag, 9 * Ly.Cout, T)), f'{tc.id} dx{i}')
            c0 += s.C
    else:
        n = Ly.N * Ly.H * Ly.W + 1
        ref = TC.backward_weight(Ly, t, T)['dW']
        mag = CR.ref(t['dW']).abs() + CR.backward_weight_terms(Ly, t, T, absolute=True)
        within(dev['dW'], ref, R.bound_r(ref, mag, n), f'{tc.id} dW')


def check_exact(tc, t, dev):
    c = tc.case
    r = TC.reference(tc, t)
    if c.mode == CC.FWD:
        expect_equal(dev['y'], r['y'], f'{tc.id} y', where)
    elif c.mode == CC.DGRAD:
        for i in range(len(c.layer.srcs)):
            expect_equal(dev[f'dx{i}'], r[f'dx{i}'], f'{tc.id} dx{i}', where)
    else:
        expect_equal(dev['dW'], r['dW'], f'{tc.id} dW', w_where)


def run_group(cases, dev, routes=None):
    """Launch every case, synchronise once, then judge every case (a failure does not hide the ones behind it)."""
    G = CR.Guard(dev)
    staged, failures = [], []
    for tc in cases:
        try:
            t, d, scratch, again = stage(tc, G)
            launch(tc, d, scratch, routes)
            if again is not None:
                launch(tc, again[0], again[1], routes)
            staged.append((tc, t, d, again))
        except AssertionError as e:
            failures.append(f'{tc.id}: {str(e)[:400]}')
        except RuntimeError as e:
            if 'HIP' in str(e) or 'octseg error -4' in str(e):      # a HIP error: nothing more is started on this GPU
                pytest.exit(f'{tc.id}: {e!r}', returncode=3)
            failures.append(f'{tc.id}: {e!r}'[:400])
    torch.cuda.synchronize()
    try:
        G.check()
    except AssertionError as e:
        failures.append(f'guards: {e}')
    for tc, t, d, again in staged:
        try:
            (check_exact if tc.case.exact else check_rounding)(tc, t, d)
            if again is not None:
                for k in CC.OUTPUTS[tc.case.mode](tc.case.layer):
                    assert torch.equal(R.bits_of(d[k]), R.bits_of(again[0][k])), f'{tc.id}: a second launch wrote another {k}'
        except AssertionError as e:
            failures.append(f'{tc.id}: {str(e)[:600]}')
    assert not failures, f'{len(failures)} failures in {len(cases)} cases:\n' + '\n'.join(failures)


@pytest.mark.parametrize('mode', [CC.FWD, CC.DGRAD, CC.WGRAD], ids=['fwd', 'dgrad', 'wgrad'])
def test_tied_pass(mode, cuda):
    run_group([tc for tc in TC.all_cases() if tc.case.mode == mode], cuda)


def test_weight_gradients_in_deterministic_mode(cuda):
    """The exact weight-gradient cases again without split-K (one writer per element of the 4x4 image's gradient): the same sums, bit for bit."""
    cases = [tc for tc in TC.all_cases() if tc.case.mode == CC.WGRAD and tc.case.exact]
    before = 1 if os.environ.get('OCTSEG_DETERMINISTIC') is not None else 0
    L.check(L.lib().octseg_set_deterministic(1))
    try:
        run_group(cases, cuda, routes={'convt16', 'mfma'})
    finally:
        L.check(L.lib().octseg_set_deterministic(before))


def test_refused_calls_write_nothing(cuda):
    """Well-formed device buffers, ill-formed descriptors: refused before any launch, and every buffer still holds what it held."""
    tcs = {tc.case.mode: tc for tc in TC.all_cases() if tc.case.name == 'm16_cs32'}
    G = CR.Guard(cuda)
    bufs, ptrs = {}, {}
    for mode, tc in tcs.items():
        t, dev, scratch, _ = stage(tc, G)
        bufs.update({f'{mode}.{k}': v for k, v in dev.items()})
        bufs[f'{mode}.scratch'] = scratch
        ptrs[mode] = {**{k: v.data_ptr() for k, v in dev.items()}, 'scratch': scratch.data_ptr()}
    before = {k: v.clone() for k, v in bufs.items()}
    Ly = tcs[CC.FWD].case.layer
    nb = CO.tied_scratch_bytes(Ly)
    lib = L.lib()

    def op(mode, layer, p, dt=L.BF16, nbytes=nb, wg=0):
        return lib.octseg_tied_layer_op(mode, dt, C.byref(CO.make_desc(layer, p, nbytes)), wg, L.stream_ptr())
    for mode in (CC.FWD, CC.DGRAD, CC.WGRAD):
        assert op(mode, Ly, ptrs[mode], dt=L.F16) == -2 and op(mode, Ly, ptrs[mode], dt=L.F32) == -2
        assert op(mode, Ly, ptrs[mode], nbytes=nb - 16) == -5
        assert op(mode, Ly, ptrs[mode], wg=-1) == -5
    narrow = copy.deepcopy(Ly); narrow.srcs[0].C = 56
    assert op(CC.FWD, narrow, ptrs[CC.FWD]) == -1
    acc = copy.deepcopy(Ly); acc.accum = (1, 0, 0, 0, 0)
    assert op(CC.FWD, acc, ptrs[CC.FWD]) == -5
    pl = copy.deepcopy(Ly); pl.pool = (1, 0, 0, 0, 0)
    assert op(CC.DGRAD, pl, ptrs[CC.DGRAD]) == -5
    assert op(CC.DGRAD, Ly, {**ptrs[CC.DGRAD], 'dx0': ptrs[CC.DGRAD]['dx0'] + 2}) == -5
    assert op(CC.WGRAD, Ly, {k: v for k, v in ptrs[CC.WGRAD].items() if k != 'dW'}) == -5
    torch.cuda.synchronize()
    G.check()
    for k, v in bufs.items():
        assert torch.equal(v if v.dtype == torch.uint8 else R.bits_of(v), before[k] if v.dtype == torch.uint8 else R.bits_of(before[k])), k
