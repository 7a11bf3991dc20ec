"""Single-launch parity of conv_mfma_kernel's 64-channel N tiles: the 2-byte 3x3 stride-1 layers with 33..64 output channels, and the K-thin data
gradients (one K chunk) that choose() gives 64-channel tiles.

Several K chunks run 16 x 16-pixel tiles on four waves of 64 pixels x 64 channels with the register-prefetch loop (run9p: one window buffer, the
next chunk's eleven window passes loaded over the nine taps).  One K chunk keeps two 32-channel wave columns on the slab ring (run9s) or, on
grids as small as these, the rolled loop: 8 x 16-pixel tiles here.  Every case has exact-arithmetic operands (tests/conv_cases.py): every output element, every slab sum and every
guard row is compared for equality with the float64 reference of tests/conv_ref.py, through the stage / launch / check helpers of
tests/test_gpu_convops.py (route asserted on the launched pointers, NaN margins, poisoned input margins, untouched slab rows outside the launch's own).

The host-only test pins the route and the slab-row count (one row per tile of the stated pixel size) without a GPU.
"""
import pytest

import conv_cases as CC
import test_gpu_convops as TG
from conv_cases import AR, A, P, Case, DENSE, FWD, DGRAD
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import convops as CO
from oct_segmentation_amd.convops import Layer

R1 = ('mfma-16',)
TILE_W = 16


def tile_h(layer):
    """Rows of the workgroup tile: 16 over several 64-channel K chunks (four waves, each 4 rows x 16 pixels x 64 channels); the one-chunk layers
    keep 2 x 2 waves of 64 x 32 on 8 rows at these grid sizes."""
    return 16 if layer.Cin > 64 else 8


def forward_cases(T):
    c = [
        # four K chunks (the slab ring wraps, three window restages): upsampled source + skip, lazy BN + ReLU, ragged tiles both ways, offset slab rows
        Case('up_skip_4chunks', FWD, T, Layer(1, 24, 40, 3, 64, [AR(192, up=1), AR(64)], pad=1, slab_row0=3), R1, ('slab',)),
        # partial N tile (40 of 64), second source off the K chunk (src_uniform = 0), partial last chunk (136 = 2 x 64 + 8)
        Case('cat72_64_n40', FWD, T, Layer(2, 24, 40, 3, 40, [AR(72), P(64)], pad=1), R1, ('slab',)),
        # whole tiles only: the block-uniform epilogue
        Case('whole_tiles', FWD, T, Layer(2, 32, 16, 3, 64, [A(128)], pad=1), R1, ('slab', 'bias')),
        Case('fold', FWD, T, Layer(1, 24, 40, 3, 64, [P(128)], pad=1, relu_out=True), R1, ('wscale', 'bias')),
        Case('fold_accum', FWD, T, Layer(1, 24, 40, 3, 64, [P(128)], pad=1, relu_out=True, accum=(1, 0, 0, 0, 0)), R1, ('wscale', 'bias')),
        # one K chunk: two 32-channel wave columns
        Case('64_64', FWD, T, Layer(1, 24, 40, 3, 64, [AR(64)], pad=1), R1, ('slab',)),
    ]
    return c


def dgrad_cases(T):
    return [
        # K-thin: K = 64, N = 192 on three 64-channel tiles, two destinations, the second accumulated
        Case('kthin_two_dst', DGRAD, T, Layer(1, 24, 40, 3, 64, [P(64), P(128)], pad=1, accum=(0, 1, 0, 0, 0)), R1, nnz=DENSE),
        # pooled + accumulated destination behind the `up` source
        Case('kthin_pooled', DGRAD, T, Layer(2, 24, 40, 3, 64, [P(64, up=1), P(64)], pad=1, accum=(1, 0, 0, 0, 0), pool=(1, 0, 0, 0, 0)), R1, nnz=DENSE),
    ]


def cases():
    c = forward_cases(CC.BF16) + forward_cases(CC.F16) + dgrad_cases(CC.BF16)
    for k in c:
        k.group = 'n64'
    return c


def test_cases_are_exact_and_route_to_16_pixel_wide_tiles():
    """No GPU: every case is routed to conv_mfma's 16-pixel tiling, and a forward's statistics slab has one row per tile (16 x 16 pixels over
    several K chunks)."""
    for case in cases():
        assert case.exact
        Ly = case.layer
        assert CO.route(case.mode, case.dt, Ly, has=case.has) == ['mfma-16'], case.id
        if case.mode == FWD:
            oh, ow = Ly.out_hw
            tiles = Ly.N * ((oh + tile_h(Ly) - 1) // tile_h(Ly)) * ((ow + TILE_W - 1) // TILE_W)
            assert CO.slab_rows(case.dt, Ly, has=case.has) == tiles, case.id
    # the f32 plan of the same layer keeps its 8-row tiles
    f32 = Layer(1, 24, 40, 3, 64, [AR(64)], pad=1)
    assert CO.slab_rows(L.F32, f32) == 3 * 3


@pytest.mark.gpu
@pytest.mark.parametrize('T', [CC.BF16, CC.F16], ids=['bf16', 'f16'])
def test_forward_n64(T, cuda):
    c = forward_cases(T)
    for k in c:
        k.group = 'n64'
    TG.run_group(c, cuda)


@pytest.mark.gpu
def test_data_gradient_n64(cuda):
    c = dgrad_cases(CC.BF16)
    for k in c:
        k.group = 'n64'
    TG.run_group(c, cuda)
