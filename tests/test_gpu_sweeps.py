"""Single-op parity of the NHWC sweep kernels (f32 / bf16 / f16) against the float64 references of tests/sweep_ref.py.

One launcher per call through octseg_sweep_op (oct_segmentation_amd/sweeps.py).  The cases, their shapes and the rule that
judges each (X exact, E element-wise, R reductions, T transcendentals: see sweep_ref.py) are listed in tests/sweep_cases.py.
Every tensor handed to the GPU is an interior view of a larger allocation with 4 KiB NaN margins either side; outputs,
slabs, scratches and "store" destinations start as NaN; after each call every margin must be untouched.

Covered launchers: bn_finalize_train / _small / _eval / _frozen, bn_act, bn_bwd_small / _reduce / _finalize / _apply (alone and chained
as the plan chains them, dy aliasing g), masked_accum, pool2x2_accum, up2_fill, relu, add2, drop_elem, merge_drop, drop_bwd, channel_sum
(vector and scalar kernels, deterministic mode on and off), tensor_stats, maxpool_fwd, maxpool_bwd_idx, bilinear_resize (which
bilinear_up forwards to), bilinear_resize_adjoint, bilinear_adjoint, bin_mean, bin_mean_bwd, image_sum, image_bcast, se_gate, se_dgate,
parity_permute, mosaic, dw_conv, dw_wgrad (deterministic mode on and off), cam_seed, dwg_fwd / dwg_bwd_data / dwg_bwd_w (K 3 | 5, stride 1 | 2,
TF "same" padding on even and odd maps, deterministic mode), bnx_fwd / bnx_bwd, sefc_fwd / sefc_bwd, GroupNorm forward (gn_act_up at up 1 | 2;
the launcher has no up = 4) and backward, dice_bwd.

pan.hip's maxpool2 and fpa_* and pab.hip's pab_* have a door of their own (octseg_fpa_op / octseg_pab_op): tests/test_gpu_blockops.py.
"""
import pytest
import torch

import sweep_cases as SC
import sweep_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import sweeps as S

pytestmark = pytest.mark.gpu


def run_case(case, dev):
    G = R.Guard(dev)
    t = {k: G.put(v) for k, v in case.ins.items()}
    for k, (shape, dtype, init) in case.outs.items():
        t[k] = G.empty(shape, dtype) if init is None else G.put(init)
    case.call(S, t)
    torch.cuda.synchronize()
    G.check()
    if case.refs is not None:
        for k, ref in case.refs().items():
            R.assert_exact(t[k], ref, f'{case.id} {k}')
    else:
        case.check({k: (None if v is None else v.cpu()) for k, v in t.items()})


@pytest.mark.parametrize('family', sorted(SC.FAMILIES))
def test_sweep_family(family, cuda):
    """Every case of the family runs (a failure does not hide the ones behind it); the report names each failing case."""
    n0 = len(R.RATIOS)
    failures = []
    cases = SC.FAMILIES[family]()
    for case in cases:
        try:
            run_case(case, cuda)
        except AssertionError as e:
            failures.append(f'{case.id}: {str(e)[:400]}')
        except Exception as e:
            if isinstance(e, RuntimeError) and ('HIP' in str(e) or 'octseg error -4' in str(e)):      # a HIP error: nothing more is started on this GPU
                pytest.exit(f'{case.id}: {e!r}', returncode=3)
            failures.append(f'{case.id}: {e!r}'[:400])
    worst = {}
    for what, dt, ratio in R.RATIOS[n0:]:
        key = ((what.split('-')[0].split(' ')[0] + ' ' + (what.split(' ')[-1] if ' ' in what else '')).strip(), dt)
        worst[key] = max(worst.get(key, 0.0), ratio)
    for (what, dt), ratio in sorted(worst.items()):
        print(f'RATIO {what} {dt} {ratio:.3f}')
    assert not failures, f'{len(failures)} of {len(cases)} cases failed:\n' + '\n'.join(failures)


def test_training_only_sweeps_refuse_f16(cuda):
    """One well-formed call per training-only op, on real device buffers, with f16: refused with OCTSEG_BAD_DTYPE and nothing is written."""
    G = R.Guard(cuda)
    bufs = [G.empty((4096,), torch.float32) for _ in range(17)]
    for op, nptrs, ia, fa in SC.TRAIN_ONLY:
        assert S.sweep_op_raw(op, L.F16, [b.data_ptr() for b in bufs[:nptrs]], ia, fa, L.stream_ptr()) == -2, op
    torch.cuda.synchronize()
    G.check()
    assert all(bool(torch.isnan(b).all()) for b in bufs)
