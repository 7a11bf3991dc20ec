"""One conv layer pass per call, with the fused descriptors the plan builds (csrc/conv_api.cpp, include/octseg.h).

They exist so that every conv route (thin, gemm1x1, conv3x3p, conv_mfma's tilings, the weight-gradient kernels) can be pinned
against a float64 reference with its fused operand and epilogue paths switched on, one launch at a time
(tests/test_gpu_convops.py); the network path uses the plan API in ``engine.py``.  ``conv_layer`` derives every buffer size
from the layer and checks the tensors against it, allocates the weight-image scratch and enqueues on the current stream;
``route`` and ``slab_rows`` ask which kernels would run and launch nothing (they also work on pointers that are never read).
"""
import ctypes as C
from dataclasses import dataclass
from typing import List, Tuple

import torch

from . import _lib as L
from .ops import _dt

FORWARD, BACKWARD_DATA, BACKWARD_WEIGHT = 0, 1, 2
ROUTES = ['thin', 'gemm1x1', 'conv3x3p', 'mfma-16', 'mfma-11', 'mfma-wideN']      # octseg_conv_route
WROUTES = ['thin', 'wgrad1x1', 'convt16', 'mfma']                                  # octseg_wgrad_route
TORCH_OF = {L.F32: torch.float32, L.BF16: torch.bfloat16, L.F16: torch.float16}


@dataclass
class Src:
    """One source of the concatenated input: C channels, stored at half resolution when `up`, read through relu?(x * scale + shift) when `affine`."""
    C: int
    up: int = 0
    affine: bool = False
    relu: bool = False


@dataclass
class Layer:
    N: int
    H: int                     # virtual input extent (after `up`)
    W: int
    R: int
    Cout: int
    srcs: List[Src]
    stride: int = 1
    pad: int = 0
    transposed: bool = False
    relu_out: bool = False
    head: bool = False
    slab_row0: int = 0
    accum: Tuple[int, ...] = (0,) * L.CONV_MAX_SRC     # per destination (forward: the first)
    pool: Tuple[int, ...] = (0,) * L.CONV_MAX_SRC

    @property
    def Cin(self):
        return sum(s.C for s in self.srcs)

    @property
    def out_hw(self):
        if self.transposed:
            return self.H * 2, self.W * 2
        return (self.H + 2 * self.pad - self.R) // self.stride + 1, (self.W + 2 * self.pad - self.R) // self.stride + 1

    def src_shape(self, i):
        s = self.srcs[i]
        return (self.N, self.H >> s.up, self.W >> s.up, s.C)

    def dst_shape(self, i):
        """Data gradient: the destination of source i (half resolution when pooled)."""
        s = self.srcs[i]
        return (self.N, self.H >> 1, self.W >> 1, s.C) if self.pool[i] else (self.N, self.H, self.W, s.C)

    @property
    def y_shape(self):
        oh, ow = self.out_hw
        return (self.N, self.Cout, oh, ow) if self.head else (self.N, oh, ow, self.Cout)

    @property
    def w_shape(self):
        return (self.R, self.R, self.Cout, self.Cin)


def scratch_bytes(layer, dt):
    return L.lib().octseg_conv2d_scratch_bytes(dt, layer.N, layer.H, layer.W, layer.Cin, layer.Cout, layer.R, layer.R)


def make_desc(layer, ptrs, nbytes_scratch=0):
    """octseg_conv_layer_desc of `layer`; ptrs: name -> device address (int) for x{i}, scale{i}, shift{i}, dx{i}, w, wscale, bias, slab, y, dy,
    dW, scratch (absent = NULL)."""
    d = L.ConvLayerDesc()
    d.N, d.H, d.W, d.Cin, d.Cout, d.R = layer.N, layer.H, layer.W, layer.Cin, layer.Cout, layer.R
    d.stride, d.pad, d.transposed, d.nsrc = layer.stride, layer.pad, int(layer.transposed), len(layer.srcs)
    for i, s in enumerate(layer.srcs[:L.CONV_MAX_SRC]):
        d.src[i].ptr, d.src[i].scale, d.src[i].shift = ptrs.get(f'x{i}'), ptrs.get(f'scale{i}'), ptrs.get(f'shift{i}')
        d.src[i].C, d.src[i].H, d.src[i].W, d.src[i].up, d.src[i].relu = s.C, layer.H >> s.up, layer.W >> s.up, s.up, int(s.relu)
        d.dst[i].ptr, d.dst[i].accum, d.dst[i].pool = ptrs.get(f'dx{i}'), int(layer.accum[i]), int(layer.pool[i])
    if 'y' in ptrs:
        d.dst[0].ptr = ptrs['y']
    d.w, d.wscale, d.bias = ptrs.get('w'), ptrs.get('wscale'), ptrs.get('bias')
    d.relu_out, d.stat_slab, d.slab_row0, d.head = int(layer.relu_out), ptrs.get('slab'), layer.slab_row0, int(layer.head)
    d.dy, d.dW, d.scratch, d.scratch_bytes = ptrs.get('dy'), ptrs.get('dW'), ptrs.get('scratch'), nbytes_scratch
    return d


def operand_names(mode, layer, has=()):
    """Names of the tensors a call of `mode` takes; `has`: which of wscale / bias / slab are present."""
    n = len(layer.srcs)
    names = []
    if mode != BACKWARD_DATA:
        names += [f'x{i}' for i in range(n)]
        for i, s in enumerate(layer.srcs):
            if s.affine:
                names += [f'scale{i}', f'shift{i}']
    if mode == FORWARD:
        names += ['w', 'y'] + [k for k in ('wscale', 'bias', 'slab') if k in has]
    elif mode == BACKWARD_DATA:
        names += ['w', 'dy'] + [f'dx{i}' for i in range(n)]
    else:
        names += ['dy', 'dW']
    return names


def fake_ptrs(mode, layer, has=()):
    """Aligned non-null stand-ins for the routing queries (nothing dereferences them)."""
    p = {k: 0x10000 * (i + 1) for i, k in enumerate(operand_names(mode, layer, has))}
    p['scratch'] = 0x400000
    return p


def route_raw(mode, dt, desc):
    r = (C.c_int * 8)()
    n = C.c_int(0)
    rc = L.lib().octseg_conv_layer_route(mode, dt, C.byref(desc), r, C.byref(n))
    return rc, [r[i] for i in range(n.value)]


def route(mode, dt, layer, ptrs=None, has=()):
    """Kernel of every launch of the pass, as names (None: a launch without taps)."""
    ptrs = fake_ptrs(mode, layer, has) if ptrs is None else {'scratch': 0x400000, **ptrs}
    rc, r = route_raw(mode, dt, make_desc(layer, ptrs, 1 << 40))
    L.check(rc)
    names = WROUTES if mode == BACKWARD_WEIGHT else ROUTES
    return [None if v < 0 else names[v] for v in r]


def slab_rows(dt, layer, ptrs=None, has=('slab',)):
    ptrs = fake_ptrs(FORWARD, layer, has) if ptrs is None else {'scratch': 0x400000, **ptrs}
    rows = C.c_int(0)
    L.check(L.lib().octseg_conv_layer_slab_rows(dt, C.byref(make_desc(layer, ptrs, 1 << 40)), C.byref(rows)))
    return rows.value


def _need(t, name, shape, dtype):
    v = t[name]
    assert v.is_cuda and v.is_contiguous(), f'{name}: a contiguous device tensor is expected'
    assert v.dtype == dtype, f'{name}: dtype {v.dtype}, expected {dtype}'
    assert tuple(v.shape) == tuple(shape), f'{name}: shape {tuple(v.shape)}, expected {tuple(shape)}'


def check_tensors(mode, layer, t, T):
    """Every tensor of the call against the size the layer implies."""
    f32 = torch.float32
    oh, ow = layer.out_hw
    if mode != BACKWARD_DATA:
        for i, s in enumerate(layer.srcs):
            _need(t, f'x{i}', layer.src_shape(i), T)
            if s.affine:
                _need(t, f'scale{i}', (s.C,), f32)
                _need(t, f'shift{i}', (s.C,), f32)
    if mode != BACKWARD_WEIGHT:
        _need(t, 'w', layer.w_shape, f32)
    if mode == FORWARD:
        _need(t, 'y', layer.y_shape, f32 if layer.head else T)
        for k in ('wscale', 'bias'):
            if k in t:
                _need(t, k, (layer.Cout,), f32)
        if 'slab' in t:
            assert t['slab'].dtype == f32 and t['slab'].dim() == 3 and t['slab'].shape[1:] == (layer.Cout, 2)
            rows = slab_rows(_DT[T], layer, {k: v.data_ptr() for k, v in t.items()}, has=('slab',))
            assert t['slab'].shape[0] >= layer.slab_row0 + rows, f'slab: {t["slab"].shape[0]} rows, the launch writes [{layer.slab_row0}, {layer.slab_row0 + rows})'
    else:
        _need(t, 'dy', (layer.N, oh, ow, layer.Cout), T)
        if mode == BACKWARD_DATA:
            for i in range(len(layer.srcs)):
                _need(t, f'dx{i}', layer.dst_shape(i), T)
        else:
            _need(t, 'dW', layer.w_shape, f32)


_DT = {v: k for k, v in TORCH_OF.items()}


def conv_layer(mode, layer, t, scratch=None):
    """Enqueue one pass of `layer` on the current stream.  t: name -> device tensor (operand_names); the element type is taken from dy / x0."""
    T = (t['dy'] if mode != FORWARD else t['x0']).dtype
    dt = _dt(t['dy'] if mode != FORWARD else t['x0'])
    t = {k: v for k, v in t.items() if v is not None}
    check_tensors(mode, layer, t, T)
    ptrs = {k: v.data_ptr() for k, v in t.items()}
    nb = 0
    if mode != BACKWARD_WEIGHT:
        nb = scratch_bytes(layer, dt)
        if scratch is None:
            scratch = torch.empty(nb, dtype=torch.uint8, device=t['w'].device)
        assert scratch.numel() >= nb
        ptrs['scratch'] = scratch.data_ptr()
    L.check(L.lib().octseg_conv_layer_op(mode, dt, C.byref(make_desc(layer, ptrs, nb)), L.stream_ptr()))
    return scratch
