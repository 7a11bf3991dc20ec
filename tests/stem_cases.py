"""Cases of the single-launch stem tests (tests/test_stemops.py on the CPU, tests/test_gpu_stemops.py on the GPU).

A case = one call of octseg_stem_op (oct_segmentation_amd/convops.py: Stem, stem()), judged as the conv cases of tests/conv_cases.py are:
  exact     normalize = 0 on integer frames in [-4, 4]; weights in {0, +-0.25, +-0.5, +-1} (coarse: {0, +-1}), wscale in {0, +-0.25, +-0.5, +-1}, bias an
            integer in [-3, 3], dy an integer in [-2, 2], dW before the call an integer in [-4, 4]: every product and every partial sum is a float32
            whatever the order, so the result equals the float64 reference rounded by the store rule, bit for bit.  density() thins the weights of
            the forwards with a slab so that each channel's sum y^2 over the whole map stays below 2^24 units; every one of the 147 taps keeps a
            non-zero weight in at least one output channel.
  rounding  uniform frames in [0, 1] normalised with the ImageNet mean and std, Gaussian weights / dy: Rule R of sweep_ref.py, n = the terms added
            per output (147 (+ bias) forward; N OH OW + 1 weight gradient).
  im2col    pure data movement plus the normalisation formula: bit for bit for any frame.
Shapes (thin.hip KSTEM walks 4 x 32-pixel tiles with at most 512 persistent workgroups):
  ragged      N 2, 36 x 88    OH 18 = 4.5 tile rows, OW 44 = 1.4 tile columns
  tiny        N 1, 8 x 8      one tile whose frame window is mostly clamped
  persistent  N 3, 198 x 432  OH 99, OW 216: 3 x 25 x 7 = 525 tiles on 512 workgroups -- 13 workgroups take two tiles, every other one prefetches
                              the clamped last tile; 512 slab rows
"""
import zlib
from dataclasses import dataclass
from typing import Tuple

import torch

from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import convops as CO
from oct_segmentation_amd.convops import Stem

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
DT = {F32: L.F32, BF16: L.BF16, F16: L.F16}
L_NAMES = {F32: 'f32', BF16: 'bf16', F16: 'f16'}
IM2COL, FWD, WGRAD = CO.STEM_IM2COL, CO.STEM_FORWARD, CO.STEM_WGRAD
STAGE_NAMES = {IM2COL: 'im2col', FWD: 'fwd', WGRAD: 'wgrad'}
SLAB_TAIL = 2          # rows allocated behind the launch's last slab row: they must stay untouched
IMAGENET = dict(normalize=True, mean=(0.485, 0.456, 0.406), std=(0.229, 0.224, 0.225))
RAGGED, TINY, PERSISTENT = (2, 36, 88), (1, 8, 8), (3, 198, 432)


@dataclass
class Case:
    name: str
    stage: int
    T: torch.dtype
    stem: Stem
    has: Tuple[str, ...] = ()              # FORWARD: of 'wscale', 'bias', 'slab'
    exact: bool = True

    @property
    def id(self):
        return f'stem.{self.name}.{STAGE_NAMES[self.stage]}.{L_NAMES[self.T]}'

    @property
    def dt(self):
        return DT[self.T]


EVAL = ('wscale', 'bias')


def forward_cases(T):
    c = [
        Case('ragged', FWD, T, Stem(*RAGGED, slab_row0=3), ('slab',)),
        Case('tiny', FWD, T, Stem(*TINY), ('slab',)),
        Case('persistent', FWD, T, Stem(*PERSISTENT), ('slab',)),
        Case('eval', FWD, T, Stem(*RAGGED, relu_out=True), EVAL),
        Case('eval_linear', FWD, T, Stem(*RAGGED), EVAL),                    # a BatchNorm without the ReLU behind it: bias, no clamp
        Case('plain', FWD, T, Stem(*TINY)),                                  # no slab, no fold
        Case('gauss', FWD, T, Stem(*RAGGED, relu_out=True, **IMAGENET), EVAL, exact=False),
        Case('gauss_train', FWD, T, Stem(*RAGGED, **IMAGENET), (), exact=False),
    ]
    return c


def wgrad_cases():
    return [
        Case('ragged', WGRAD, BF16, Stem(*RAGGED)),
        Case('tiny', WGRAD, BF16, Stem(*TINY)),
        Case('persistent', WGRAD, BF16, Stem(*PERSISTENT)),
        Case('gauss', WGRAD, BF16, Stem(*RAGGED, **IMAGENET), exact=False),
    ]


def im2col_cases():
    c = []
    for T in (F32, BF16, F16):
        for k, p, KP in CO.STEM_KINDS:
            c.append(Case(f'k{k}p{p}', IM2COL, T, Stem(2, 12, 20, ksize=k, pad=p, KP=KP)))
            c.append(Case(f'k{k}p{p}_norm', IM2COL, T, Stem(2, 12, 20, ksize=k, pad=p, KP=KP, **IMAGENET)))
    return c


def all_cases():
    return forward_cases(BF16) + forward_cases(F16) + wgrad_cases() + im2col_cases()


# ------------------------------------------------------------------------------------------------ operands
def _gen(case):
    return torch.Generator().manual_seed(zlib.crc32(case.id.encode()))


def _choice(values, shape, g):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), shape, generator=g)]


def _ints(shape, g, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.float64)


def density(case):
    """(coarse, nnz) of an exact forward.  With a slab, a channel's sum y^2 over the whole map has to stay below 2^24 units (unit = the square of the
    products' granularity: 1/16 with quarter weights on integer frames, 1 with coarse weights in {0, +-1}).  With k non-zero weights per output
    channel E[y^2] is about k E[x^2] E[w^2], E[x^2] = 20 / 3 for integers in [-4, 4]; a factor 6 covers the worst channel (conv_cases.density).
    Without a slab half of the 147 weights are non-zero."""
    if 'slab' not in case.has:
        return False, None
    oh, ow = case.stem.out_hw
    budget = 2.0 ** 24 / (case.stem.N * oh * ow)
    k_fine = int(budget / 16 / (20 / 3 * 0.44 * 6))
    if k_fine >= 8:
        return False, min(k_fine, 73)
    return True, max(3, int(budget / (20 / 3 * 6)))


def _weights(case, g):
    shape = (CO.STEM_COUT, CO.STEM_KP)
    if not case.exact:
        return (torch.randn(shape, generator=g, dtype=torch.float64) * 0.1).to(torch.float32)
    coarse, nnz = density(case)
    w = _choice([-1, 1] if coarse else [-1, -0.5, -0.25, 0.25, 0.5, 1], shape, g)
    if nnz is None:
        keep = torch.rand(shape, generator=g, dtype=torch.float64) < 0.5
    else:
        keep = torch.zeros(shape, dtype=torch.bool)
        for o in range(CO.STEM_COUT):
            keep[o, torch.randperm(147, generator=g)[:max(nnz - 3, 0)]] = True
            for j in range(3):                                  # 64 x 3 = 192 >= 147: every tap has a non-zero weight in some channel
                keep[o, (o + 64 * j) % 147] = True
    # columns 147..159 are padding the kernels must never read: a weight there would show in every output
    w = (w * keep).to(torch.float32)
    w[:, 147:] = 64.0
    return w.contiguous()


def make_operands(case):
    """name -> CPU tensor: every input, and every destination with its initial content (NaN where the launch stores, known values where it
    accumulates); 'slab' has slab_row0 + rows + SLAB_TAIL rows of NaN."""
    g = _gen(case)
    st, T = case.stem, case.T
    nan = float('nan')
    t = {}
    if case.stage == IM2COL or not case.exact:
        t['img'] = torch.rand(st.img_shape, generator=g, dtype=torch.float64).to(torch.float32)
    else:
        t['img'] = _ints(st.img_shape, g, -4, 4).to(torch.float32)
    if case.stage == IM2COL:
        t['col'] = torch.full(st.col_shape, nan, dtype=T)
    elif case.stage == FWD:
        t['w'] = _weights(case, g)
        if 'wscale' in case.has:
            t['wscale'] = (_choice([-1, -0.5, 0.25, 0.5, 1, 1, 0], (64,), g) if case.exact else torch.randn((64,), generator=g, dtype=torch.float64)).to(torch.float32)
        if 'bias' in case.has:
            t['bias'] = (_ints((64,), g, -3, 3) if case.exact else torch.randn((64,), generator=g, dtype=torch.float64)).to(torch.float32)
        if 'slab' in case.has:
            t['slab'] = torch.full((st.slab_row0 + CO.stem_slab_rows(st) + SLAB_TAIL, 64, 2), nan, dtype=torch.float32)
        t['y'] = torch.full(st.y_shape, nan, dtype=T)
    else:
        t['dy'] = (_ints(st.y_shape, g, -2, 2) if case.exact else torch.randn(st.y_shape, generator=g, dtype=torch.float64).to(torch.float32)).to(T)
        t['dW'] = _ints(st.w_shape, g, -4, 4).to(torch.float32)
    return t
