"""Cases of the single-launch conv tests (tests/test_convops.py on the CPU, tests/test_gpu_convops.py on the GPU).

A case = one call of octseg_conv_layer_op: the layer, the mode, the storage type, which optional operands it carries, the route every
launch must take (asserted through octseg_conv_layer_route; the eligibility constants are those of the *_eligible functions in csrc/) and
how the result is judged:
  exact     operands chosen so that every product and every partial sum is a float32 whatever the order (activations: integers in
            [-4, 4]; scale in {-1, 0.5, 1, 2}, shift a non-zero integer in [-3, 3]: every affine value a half-integer below 12; weights and
            wscale in {0, +-0.25, +-0.5, +-1}; bias an integer in [-3, 3]; dy an integer in [-2, 2]; accumulated destinations integers
            in [-4, 4]).  The result is then fully determined: bit-for-bit equality with the float64 reference rounded by the store rule.
            density() thins the weights of the forwards (non-zero entries per output channel) so that the BatchNorm sums stay below 2^24 units.
  rounding  Gaussian operands (T-representable, the affine exact in float32 by construction: power-of-two scale, quarter-integer shift).
            |got - ref| <= n eps32 sum|terms| + half an ulp of T at the result (Rule R of sweep_ref.py), n = the contraction length.
Shapes are the smallest at which the route is still eligible and can still go wrong (ragged tiles, partial K chunks, partial N tiles,
sources off the chunk boundary, more than one workgroup, persistent workgroups with more than one tile).
"""
import zlib
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import convops as CO
from oct_segmentation_amd.convops import Layer, Src

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
FWD, DGRAD, WGRAD = CO.FORWARD, CO.BACKWARD_DATA, CO.BACKWARD_WEIGHT
MODE_NAMES = {FWD: 'fwd', DGRAD: 'dgrad', WGRAD: 'wgrad'}
SLAB_TAIL = 2          # rows allocated behind the launch's last slab row: they must stay untouched


@dataclass
class Case:
    name: str
    mode: int
    T: torch.dtype
    layer: Layer
    route: Tuple[Optional[str], ...]       # per launch
    has: Tuple[str, ...] = ()              # of 'wscale', 'bias', 'slab'
    exact: bool = True
    nnz: Optional[int] = None              # non-zero weights per output channel (None: density() decides)
    group: str = ''

    @property
    def id(self):
        return f'{self.group}.{self.name}.{MODE_NAMES[self.mode]}.{L_NAMES[self.T]}'

    @property
    def dt(self):
        return DT[self.T]

    @property
    def rule(self):
        """Store rule of the route (csrc/kernels.h): thin.hip stores its accumulators straight from registers."""
        return 'direct' if self.route[0] == 'thin' else 'staged'

    @property
    def features(self):
        f = set()
        for s in self.layer.srcs:
            if s.affine:
                f.add('affine_relu' if s.relu else 'affine')
            if s.up:
                f.add('up')
        if 'slab' in self.has:
            f.add('slab')
        if 'wscale' in self.has and 'bias' in self.has and self.layer.relu_out:
            f.add('eval_fold')
        return f


DENSE = -1   # Case.nnz: no zero weights, and weights and dy drawn with a positive mean (still from the exact sets), so that the sums grow with the
             # contraction length: even thin.hip's short contractions (at most 32 x 9 terms) then leave bf16's 8 bits (|v| >= 64 in quarters),
             # and an accumulated or pooled destination tells the two store rules of kernels.h apart
DT = {F32: L.F32, BF16: L.BF16, F16: L.F16}
L_NAMES = {F32: 'f32', BF16: 'bf16', F16: 'f16'}


def A(C, up=0):
    return Src(C, up, True, False)


def AR(C, up=0):
    return Src(C, up, True, True)


def P(C, up=0):
    return Src(C, up, False, False)


# ------------------------------------------------------------------------------------------------ the cases
def _mfma16(T):
    r1, r4 = ('mfma-16',), ('mfma-16',) * 4
    c = [
        # 3x3 on ragged tiles (24 x 40: one and a half 16-row tiles, two and a half 16-pixel columns), padded, slab rows offset
        Case('ragged', FWD, T, Layer(2, 24, 40, 3, 16, [AR(32)], pad=1, slab_row0=3), r1, ('slab',)),
        Case('dense8x8', FWD, T, Layer(1, 8, 8, 3, 16, [AR(32)], pad=1), r1, ('slab',)),                   # 64 pixels: dense weights, y beyond bf16's 8 bits
        Case('ragged_affine', FWD, T, Layer(2, 24, 40, 3, 16, [A(32)], pad=1), r1, ('slab', 'bias')),
        Case('stride2', FWD, T, Layer(2, 24, 40, 3, 16, [AR(32)], stride=2, pad=1), r1, ('slab',)),
        Case('cat24_40', FWD, T, Layer(2, 24, 40, 3, 32, [AR(24), P(40)], pad=1), r1, ('slab',)),          # second source off the K chunk: src_uniform = 0
        Case('cat64_64', FWD, T, Layer(1, 24, 40, 3, 32, [A(64), AR(64)], pad=1), r1),
        Case('decoder', FWD, T, Layer(2, 24, 40, 3, 16, [AR(32, up=1), AR(16)], pad=1, slab_row0=1), r1, ('slab',)),
        Case('head3', FWD, T, Layer(1, 24, 40, 3, 3, [AR(32)], pad=1, head=True), r1, ('bias',)),
        Case('fold', FWD, T, Layer(2, 24, 40, 3, 16, [P(32)], pad=1, relu_out=True), r1, ('wscale', 'bias')),
        Case('accum', FWD, T, Layer(1, 24, 40, 3, 16, [AR(32)], pad=1, accum=(1, 0, 0, 0, 0)), r1),
        Case('1x1_flat', FWD, T, Layer(2, 24, 40, 1, 16, [AR(32)]), r1, ('slab',)),                          # 1920 pixels: flattened to 16-pixel rows
        Case('1x1_odd', FWD, T, Layer(1, 5, 7, 1, 16, [AR(32)], slab_row0=3), r1, ('slab',)),               # 35 pixels: not flattened
        Case('convT', FWD, T, Layer(1, 12, 20, 4, 16, [AR(32)], stride=2, pad=1, transposed=True, slab_row0=3), r4, ('slab',)),
        Case('convT_wide', FWD, T, Layer(1, 12, 20, 4, 72, [AR(64)], stride=2, pad=1, transposed=True, slab_row0=3), r4, ('slab',)),   # 2-byte types: the four-tap masked loop
        # data gradients: two destinations, one pooled behind an `up` source and accumulated; stride 2 (four parity launches)
        Case('decoder', DGRAD, T, Layer(2, 24, 40, 3, 32, [P(32, up=1), P(16)], pad=1, accum=(1, 0, 0, 0, 0), pool=(1, 0, 0, 0, 0)), r1, nnz=DENSE),
        Case('cat24_40', DGRAD, T, Layer(1, 24, 40, 3, 32, [P(24), P(40)], pad=1, accum=(0, 1, 0, 0, 0)), r1, nnz=DENSE),
        Case('stride2', DGRAD, T, Layer(1, 24, 40, 3, 16, [P(32)], stride=2, pad=1), r4),
        Case('convT', DGRAD, T, Layer(1, 12, 20, 4, 64, [P(32)], stride=2, pad=1, transposed=True, accum=(1, 0, 0, 0, 0)), r1, nnz=DENSE),
    ]
    return c


def _mfma11(T):
    r = ('mfma-11',)
    c = [
        Case('33x55', FWD, T, Layer(2, 33, 55, 3, 192, [AR(128)], pad=1, slab_row0=3), r, ('slab',)),
        Case('11x11', FWD, T, Layer(1, 11, 11, 3, 192, [A(128)], pad=1), r, ('slab',)),
        Case('decoder', FWD, T, Layer(1, 22, 22, 3, 72, [AR(64, up=1), P(72)], pad=1), r, ('slab',)),       # second source off the chunk; partial N tile
        Case('fold', FWD, T, Layer(1, 11, 22, 3, 72, [P(64)], pad=1, relu_out=True), r, ('wscale', 'bias')),
        Case('accum', FWD, T, Layer(1, 11, 11, 3, 72, [AR(64)], pad=1, accum=(1, 0, 0, 0, 0)), r),
    ]
    if T == BF16:
        c.append(Case('two_dst', DGRAD, T, Layer(1, 22, 11, 3, 64, [P(64), P(72)], pad=1, accum=(1, 0, 0, 0, 0)), r, nnz=DENSE))
    return c


def _gemm1x1(T):
    r = ('gemm1x1',)
    c = [
        Case('ragged', FWD, T, Layer(3, 7, 5, 1, 40, [AR(128)], slab_row0=3), r, ('slab',)),                # 105 rows: ragged M, partial N tile
        Case('256_320', FWD, T, Layer(2, 12, 12, 1, 320, [A(256)]), r, ('slab',)),
        Case('plain', FWD, T, Layer(3, 7, 5, 1, 40, [P(128)]), r, ('bias',)),
        Case('fold', FWD, T, Layer(3, 7, 5, 1, 40, [P(128)], relu_out=True), r, ('wscale', 'bias')),
        Case('accum', FWD, T, Layer(3, 7, 5, 1, 40, [AR(64)], accum=(1, 0, 0, 0, 0)), r),
    ]
    if T == BF16:
        c.append(Case('accum', DGRAD, T, Layer(3, 7, 5, 1, 256, [P(40)], accum=(1, 0, 0, 0, 0)), r, nnz=DENSE))       # into a non-zero destination
        c.append(Case('store', DGRAD, T, Layer(2, 12, 12, 1, 64, [P(72)]), r))
    return c


def _conv3x3p(T):
    r = ('conv3x3p',)
    # 4 x 128 x 128 with two N tiles = 512 items: the smallest grid the persistent kernel takes (two tiles per workgroup)
    c = [Case('128_136', FWD, T, Layer(4, 128, 128, 3, 136, [AR(128)], pad=1, slab_row0=3), r, ('slab',))]
    if T == BF16:
        c += [
            Case('decoder', FWD, T, Layer(4, 128, 128, 3, 136, [AR(128, up=1), A(64)], pad=1), r, ('slab',)),
            Case('cat96_96', FWD, T, Layer(4, 128, 128, 3, 136, [AR(96), P(96)], pad=1), r, ('slab',)),       # src_uniform = 0
            # K = 136: a partial third K chunk; destinations: pooled + accumulated behind the `up` source, plain for the skip
            Case('decoder', DGRAD, T, Layer(4, 128, 128, 3, 136, [P(128, up=1), P(64)], pad=1, accum=(1, 0, 0, 0, 0), pool=(1, 0, 0, 0, 0)), r),
        ]
    else:
        c.append(Case('fold', FWD, T, Layer(4, 128, 128, 3, 136, [P(128)], pad=1, relu_out=True), r, ('wscale', 'bias')))
    return c


def _thin(T):
    r1, r4 = ('thin',), ('thin',) * 4
    c = [
        Case('16_16', FWD, T, Layer(1, 64, 64, 3, 16, [AR(16)], pad=1, slab_row0=3), r1, ('slab',)),     # exactly 4096 pixels
        Case('32_16', FWD, T, Layer(1, 80, 72, 3, 16, [A(32)], pad=1), r1, ('slab', 'bias')),            # ragged: 72 = 2 1/4 tiles
        Case('16_32', FWD, T, Layer(1, 80, 72, 3, 32, [AR(16)], pad=1), r1, ('slab',)),
        Case('up', FWD, T, Layer(1, 64, 64, 3, 16, [AR(16, up=1)], pad=1), r1, ('slab',)),
        Case('1x1', FWD, T, Layer(1, 64, 64, 1, 32, [AR(16)], slab_row0=3), r1, ('slab',)),
        Case('convT', FWD, T, Layer(1, 64, 64, 4, 16, [AR(16)], stride=2, pad=1, transposed=True, slab_row0=3), r4, ('slab',)),
        Case('head3', FWD, T, Layer(1, 64, 64, 3, 3, [AR(16)], pad=1, head=True), r1, ('bias',)),
        Case('fold', FWD, T, Layer(1, 64, 64, 3, 16, [P(16)], pad=1, relu_out=True), r1, ('wscale', 'bias')),
        Case('accum', FWD, T, Layer(1, 80, 72, 3, 16, [AR(32)], pad=1, accum=(1, 0, 0, 0, 0)), r1),
    ]
    if T == BF16:
        c += [
            Case('up_pool', DGRAD, T, Layer(1, 64, 64, 3, 32, [P(16, up=1)], pad=1, accum=(1, 0, 0, 0, 0), pool=(1, 0, 0, 0, 0)), r1, nnz=DENSE),
            Case('up_pool_store', DGRAD, T, Layer(1, 80, 72, 3, 16, [P(32, up=1)], pad=1, pool=(1, 0, 0, 0, 0)), r1, nnz=DENSE),
            Case('accum', DGRAD, T, Layer(1, 80, 72, 3, 32, [P(16)], pad=1, accum=(1, 0, 0, 0, 0)), r1, nnz=DENSE),
        ]
    return c


def _wgrad(T):
    m1, m4 = ('mfma',), ('mfma',) * 4
    c = [
        # conv_mfma's weight gradient with 1, 4 and 9 taps, two concatenated sources, an `up` source, stride 2: every one recomputes the virtual input
        Case('1tap', WGRAD, T, Layer(2, 24, 40, 1, 16, [AR(24)]), m1),
        Case('1tap_odd', WGRAD, T, Layer(1, 5, 7, 1, 16, [AR(24)]), m1),
        Case('4tap', WGRAD, T, Layer(1, 12, 20, 4, 16, [AR(16)], stride=2, pad=1, transposed=True), m4),
        Case('9tap', WGRAD, T, Layer(2, 24, 40, 3, 16, [AR(32)], pad=1), m1),
        Case('9tap_s2', WGRAD, T, Layer(1, 24, 40, 3, 16, [AR(32)], stride=2, pad=1), m1),
        Case('cat', WGRAD, T, Layer(1, 24, 40, 3, 32, [AR(24), A(40)], pad=1), m1),
        Case('decoder', WGRAD, T, Layer(1, 24, 40, 3, 16, [AR(32, up=1), P(16)], pad=1), m1),
    ]
    if T == BF16:
        c += [
            Case('thin3x3', WGRAD, T, Layer(1, 64, 64, 3, 16, [AR(16)], pad=1), ('thin',)),
            Case('thin3x3_32', WGRAD, T, Layer(1, 80, 72, 3, 16, [AR(32, up=1)], pad=1), ('thin',)),
            Case('thin1x1', WGRAD, T, Layer(1, 64, 64, 1, 32, [AR(16)]), ('thin',)),
            Case('w1x1', WGRAD, T, Layer(3, 20, 20, 1, 64, [AR(192)]), ('wgrad1x1',)),                       # 1200 pixels = 75 rows of 16
            Case('w1x1_cat', WGRAD, T, Layer(3, 20, 20, 1, 64, [AR(128), A(64)]), ('wgrad1x1',)),
            Case('convt16', WGRAD, T, Layer(2, 12, 20, 4, 160, [AR(96)], stride=2, pad=1, transposed=True), ('convt16',)),
        ]
    return c


def _rounding(T):
    """One Gaussian case per route: forward with an affine-and-ReLU source (no slab: the exact cases carry the statistics), and the weight gradients."""
    c = [Case('m16', FWD, T, Layer(2, 24, 40, 3, 32, [AR(24), A(40)], pad=1), ('mfma-16',), ('bias',), exact=False)]
    if T != F16:
        c.append(Case('m16', WGRAD, T, Layer(2, 24, 40, 3, 16, [AR(32)], pad=1), ('mfma',), exact=False))
    if T == F32:
        return c
    c += [
        Case('m11', FWD, T, Layer(2, 33, 55, 3, 192, [AR(128)], pad=1), ('mfma-11',), ('bias',), exact=False),
        Case('gemm1x1', FWD, T, Layer(3, 7, 5, 1, 40, [AR(128)]), ('gemm1x1',), exact=False),
        Case('conv3x3p', FWD, T, Layer(4, 128, 128, 3, 136, [AR(128)], pad=1), ('conv3x3p',), exact=False),
        Case('thin', FWD, T, Layer(1, 80, 72, 3, 16, [AR(32)], pad=1), ('thin',), ('bias',), exact=False),
    ]
    if T == BF16:
        c += [
            Case('thin', WGRAD, T, Layer(1, 64, 64, 3, 16, [AR(16)], pad=1), ('thin',), exact=False),
            Case('w1x1', WGRAD, T, Layer(3, 20, 20, 1, 64, [AR(192)]), ('wgrad1x1',), exact=False),
            Case('convt16', WGRAD, T, Layer(2, 12, 20, 4, 160, [AR(96)], stride=2, pad=1, transposed=True), ('convt16',), exact=False),
        ]
    return c


# group name -> (maker, storage types)
GROUPS = {
    'mfma16': (_mfma16, (F32, BF16)),
    'mfma11': (_mfma11, (BF16, F16)),
    'gemm1x1': (_gemm1x1, (BF16, F16)),
    'conv3x3p': (_conv3x3p, (BF16, F16)),
    'thin': (_thin, (BF16, F16)),
    'wgrad': (_wgrad, (F32, BF16)),
    'rounding': (_rounding, (F32, BF16, F16)),
}
GROUP_PARAMS = [(g, T) for g, (_, types) in GROUPS.items() for T in types]
GROUP_IDS = [f'{g}-{L_NAMES[T]}' for g, T in GROUP_PARAMS]


def group_cases(group, T):
    cases = GROUPS[group][0](T)
    for c in cases:
        c.group = group
    return cases


def all_cases():
    return [c for g, T in GROUP_PARAMS for c in group_cases(g, T)]


# mfma-wideN (256 -> 256 on a grid of >= 1024 workgroups, e.g. 4 x 248 x 248) has no case: its float64 CPU reference is 145 GMAC, tens of seconds.
# It stays with tests/test_gpu_ops.py's large shapes and the whole-network tests.
# Forward routes x fused features a route is eligible for (gemm1x1_eligible refuses `up`; everything else takes every feature):
FEATURES = ('affine', 'affine_relu', 'up', 'slab', 'eval_fold')
FORWARD_ROUTES = ('thin', 'gemm1x1', 'conv3x3p', 'mfma-16', 'mfma-11')
INELIGIBLE = {('gemm1x1', 'up')}


# ------------------------------------------------------------------------------------------------ operands
def _gen(case):
    return torch.Generator().manual_seed(zlib.crc32(case.id.encode()))


def _choice(values, shape, g):
    v = torch.tensor(values, dtype=torch.float64)
    return v[torch.randint(0, len(values), shape, generator=g)]


def _ints(shape, g, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).to(torch.float64)


def density(case):
    """(coarse, nnz) of an exact case.  A forward's per-channel sum y^2 over the whole map has to stay below 2^24 units (unit = the square of the
    products' granularity: 1/64 with quarter weights and half-integer activations), so the larger the map the thinner the weights: with k
    non-zero weights per output channel E[y^2] is about k E[x^2] E[w^2] <= k 16 E[w^2]; a factor 6 covers the worst channel and the bias.
    Where that leaves fewer than 4 entries the case turns coarse -- weights in {0, +-1}, scales in {-1, 1, 2}: the unit is 1.  Gradients carry
    no statistics: about half of the weights are non-zero there."""
    Ly = case.layer
    K = Ly.R * Ly.R * Ly.Cin
    if case.nnz is not None or case.mode != FWD:
        return False, case.nnz
    oh, ow = Ly.out_hw
    budget = 2.0 ** 24 / (Ly.N * oh * ow)
    k_fine = int(budget / 64 / (16 * 0.44 * 6))
    if k_fine >= min(4, K // 2):
        return False, (None if k_fine >= K // 2 else k_fine)
    return True, max(1, min(K // 2, int(budget / (16 * 6))))


def _weights(case, g):
    Ly = case.layer
    shape = Ly.w_shape
    if not case.exact:
        return (torch.randn(shape, generator=g, dtype=torch.float64) * 0.25).to(torch.float32).to(case.T).to(torch.float32)
    coarse, nnz = density(case)
    w = _choice([1, 1, 0.5, 0.25, -0.25] if nnz == DENSE else [-1, 1] if coarse else [-1, -0.5, -0.25, 0.25, 0.5, 1], shape, g)
    K = Ly.R * Ly.R * Ly.Cin
    if nnz == DENSE:
        keep = torch.ones(shape, dtype=torch.bool)
    elif nnz is None:
        keep = torch.rand(shape, generator=g, dtype=torch.float64) < 0.5
    else:   # nnz entries per output channel, spread over taps and input channels (the last input channels included: a dropped K tail shows)
        keep = torch.zeros((Ly.Cout, K), dtype=torch.bool)
        for o in range(Ly.Cout):
            idx = torch.randperm(K, generator=g)[:nnz]
            keep[o, idx] = True
            keep[o, (o * 7) % Ly.R ** 2 * Ly.Cin + Ly.Cin - 1 - o % 8] = True
        keep = keep.view(Ly.Cout, Ly.R, Ly.R, Ly.Cin).permute(1, 2, 0, 3)
    return (w * keep).to(torch.float32).contiguous()


def make_operands(case):
    """name -> CPU tensor: every input, and every destination with its initial content (NaN where the launch stores, known values where it
    accumulates); 'slab' has case.layer.slab_row0 + rows + SLAB_TAIL rows of NaN (rows: CO.slab_rows)."""
    g = _gen(case)
    Ly, T = case.layer, case.T
    t = {}
    oh, ow = Ly.out_hw
    nan = float('nan')
    if case.mode != DGRAD:
        for i, s in enumerate(Ly.srcs):
            shape = Ly.src_shape(i)
            if case.exact:
                t[f'x{i}'] = _ints(shape, g, -4, 4).to(T)
                if s.affine:
                    t[f'scale{i}'] = _choice([-1, 1, 2] if density(case)[0] else [-1, 0.5, 1, 2], (s.C,), g).to(torch.float32)
                    t[f'shift{i}'] = _choice([-3, -2, -1, 1, 2, 3], (s.C,), g).to(torch.float32)     # never 0: a padding pixel that receives the affine shows
            else:
                x = torch.randn(shape, generator=g, dtype=torch.float64).to(torch.float32).to(T).to(torch.float64)
                t[f'x{i}'] = torch.where(x.abs() < 2.0 ** -8, torch.zeros_like(x), x).to(T)            # (keeps x * scale + shift exact in float32)
                if s.affine:
                    t[f'scale{i}'] = _choice([-1, 0.5, 1, 2], (s.C,), g).to(torch.float32)
                    t[f'shift{i}'] = _choice([-0.75, -0.5, -0.25, 0.25, 0.5, 1], (s.C,), g).to(torch.float32)
    if case.mode != WGRAD:
        t['w'] = _weights(case, g)
    if case.mode == FWD:
        if 'wscale' in case.has:
            t['wscale'] = _choice([-1, 1, 1, 0] if density(case)[0] else [-1, -0.5, 0.25, 0.5, 1, 1, 0], (Ly.Cout,), g).to(torch.float32)
        if 'bias' in case.has:
            t['bias'] = (_ints((Ly.Cout,), g, -3, 3) if case.exact else torch.randn((Ly.Cout,), generator=g, dtype=torch.float64)).to(torch.float32)
        if 'slab' in case.has:
            rows = CO.slab_rows(case.dt, Ly, has=case.has)
            t['slab'] = torch.full((Ly.slab_row0 + rows + SLAB_TAIL, Ly.Cout, 2), nan, dtype=torch.float32)
        yT = torch.float32 if Ly.head else T
        t['y'] = _ints(Ly.y_shape, g, -4, 4).to(yT) if Ly.accum[0] else torch.full(Ly.y_shape, nan, dtype=yT)
    else:
        shape = (Ly.N, oh, ow, Ly.Cout)
        t['dy'] = (_choice([2, 2, 1, 1, 0, -1], shape, g) if case.nnz == DENSE else _ints(shape, g, -2, 2)).to(T) if case.exact else torch.randn(shape, generator=g, dtype=torch.float64).to(torch.float32).to(T)
        if case.mode == DGRAD:
            for i in range(len(Ly.srcs)):
                ds = Ly.dst_shape(i)
                t[f'dx{i}'] = _ints(ds, g, -4, 4).to(T) if Ly.accum[i] else torch.full(ds, nan, dtype=T)
        else:
            t['dW'] = _ints(Ly.w_shape, g, -4, 4).to(torch.float32)
    return t


OUTPUTS = {FWD: lambda Ly: ['y'], DGRAD: lambda Ly: [f'dx{i}' for i in range(len(Ly.srcs))], WGRAD: lambda Ly: ['dW']}
