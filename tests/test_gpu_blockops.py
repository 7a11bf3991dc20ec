"""Single-stage parity of pan.hip's pyramid kernels and pab.hip's attention kernels against the float64 references of tests/block_ref.py.

One launcher per call through octseg_fpa_op / octseg_pab_op (oct_segmentation_amd/blockops.py).  The cases, their shapes and the rule
that judges each (X exact, E element-wise, R reductions, T transcendentals: see sweep_ref.py) are listed in tests/block_cases.py.  Every
tensor handed to the GPU is an interior view of a larger allocation with 4 KiB NaN margins either side; outputs and scratches start as
NaN, accumulated destinations as known non-zero values; after each case every margin must be untouched and every owned element finite.

Covered launchers: maxpool2 (forward; backward with accum 0 | 1), fpa_in_fwd, fpa_in_bwd (both kernels), fpa_pyr_fwd (train | eval: each of
its phases against the float64 reference of that phase on the kernel's own input, read back from the scratch; the 12 statistics; the
running statistics; a second launch bit for bit), fpa_pyr_bwd (against float64 autograd; a second launch bit for bit), fpa_mix, the eight
FPA stages chained with the plan's scratch offsets, pab_gemm (the six stride sets of the plan, tails in M, N and K, accum), pab_softmax,
pab_mix, and the PAB stages chained as the plan chains them.

Measured worst error / bound ratios (MI355X; "RATIO" lines of the run; Rules E and R: every one must be <= 1; Rule T: <= 4) and the pyramid backward's yardstick
distances are recorded in MEASURED below.
"""
import pytest
import torch

import block_cases as BC
import sweep_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import blockops as B

pytestmark = pytest.mark.gpu

MEASURED = """
Worst error / bound per op and dtype (Rules E and R; 1 = at the bound):
  fpa_in_fwd      f32 0.001  bf16 0.001  f16 0.001        fpa_in_bwd      f32 0.347  bf16 0.98 (the storage rounding of dp)
  fpa_mix_fwd     f32 0.198  bf16 0.992  f16 0.987        fpa_mix_bwd     f32 0.247  bf16 0.98
  pyr_conv3 | 5 | 7   0.116 | 0.069 | 0.044               pyr_bn_relu 0.260   pyr_resize 0.182   pyr_add 0.241   (float32 whatever the dtype)
  pab_gemm        f32 0.232  bf16 0.989  f16 0.204        pab_softmax_bwd 0.242                  pab_chain (per stage) f32 0.62  bf16 0.992
  (ratios near 1 in bf16 / f16 are the rounding to the storage type itself: half a unit in the last place of T is the bound's first term)
Rule T (kernel's distance from float64 / torch float32's; at most 4): pyramid rstd 1.000 (0.07 .. 1.0), pab_softmax_fwd 1.686 (spread +-200, n = 81),
  pab_chain softmax 0.78.
Pyramid backward, largest distance from float64 autograd over all 23 gradient tensors (kernel | torch float32 autograd on the CPU):
  2 x 8 x 8     1.03e-06 | 4.31e-06        3 x 22 x 14   6.15e-06 | 6.39e-06        2 x 16 x 24   5.21e-06 | 7.84e-06
  worst kernel / max(4 x yardstick, 16 eps32 max|ref|) of one tensor: 0.868 (dbeta of down2, 2 x 8 x 8: 3.19e-07 against the floor of 3.67e-07).
FPA chain (2 x 8 x 8 x 16), worst of one tensor: f32 0.455, bf16 0.448.  The level-3 BatchNorms see two values each there: before pyr_bn_relu_bwd
  took its mean again in double, the bf16 case gave d b of down3.2 (zero on paper) 5.68e-04 away (allowed 1e-06); now 0.
PAB chain against float64 autograd: y, dcenter, dtop, dbottom within 0.25 (bf16: the storage rounding) / 0.2 (f32) of the allowance.
The file runs in 1.3 s.
"""


def run_case(case, dev):
    G = R.Guard(dev)
    t = {k: G.put(v) for k, v in case.ins.items()}
    for k, (shape, dtype, init) in case.outs.items():
        t[k] = G.empty(shape, dtype) if init is None else G.put(init)
    case.call(B, t)
    torch.cuda.synchronize()
    G.check()
    if case.refs is not None:
        for k, ref in case.refs().items():
            R.assert_exact(t[k], ref, f'{case.id} {k}')
    else:
        case.check({k: (None if v is None else v.cpu()) for k, v in t.items()})


@pytest.mark.parametrize('family', sorted(BC.FAMILIES))
def test_block_family(family, cuda):
    """Every case of the family runs (a failure does not hide the ones behind it); the report names each failing case."""
    n0 = len(R.RATIOS)
    failures = []
    cases = BC.FAMILIES[family]()
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
        key = (what.split(' ')[0], dt)
        worst[key] = max(worst.get(key, 0.0), ratio)
    for (what, dt), ratio in sorted(worst.items()):
        print(f'RATIO {what} {dt} {ratio:.3f}')
    assert not failures, f'{len(failures)} of {len(cases)} cases failed:\n' + '\n'.join(failures)


def test_training_only_stages_refuse_f16(cuda):
    """One well-formed call per training-only stage, on real device buffers, with f16: refused with OCTSEG_BAD_DTYPE and nothing is written."""
    G = R.Guard(cuda)
    bufs = [G.empty((4096,), torch.float32) for _ in range(8)]
    a = [b.data_ptr() for b in bufs]
    for stage in ('maxpool2_bwd', 'in_bwd', 'pyr_bwd', 'mix_bwd'):
        d = L.FpaDesc(N=1, H=8, W=8, C=8, K=7, x=a[0], dp=a[1], dx=a[2], p=a[0], dy=a[3], w=a[4], dw=a[5], db=a[6], scratch=a[0], scratch_floats=4096,
                      gscratch=a[1], gscratch_floats=4096, duu=a[2], uu=a[0], mid=a[1], g=a[2], dmid=a[3])
        assert B.fpa_op_raw(stage, L.F16, d, L.stream_ptr()) == -2, stage
    for stage in ('softmax_bwd', 'mix_bwd'):
        d = L.PabDesc(S=a[0], P=a[1], batch=1, n=64, dy=a[0], dM=a[1], N=1, HW=8, C=8)
        assert B.pab_op_raw(stage, L.F16, d, L.stream_ptr()) == -2, stage
    torch.cuda.synchronize()
    G.check()
    assert all(bool(torch.isnan(b).all()) for b in bufs)
