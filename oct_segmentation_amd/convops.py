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


# ------------------------------------------------------------------------------------------------ the tied decoder layer (octseg_tied_layer_op)
# A tied layer is a Layer(N, H, W, 3, Cout, [Src(Ca, up=1, ...), Src(C1), ...], pad=1): src 0 stored at H / 2 x W / 2.  accum[0] is the
# low-resolution gradient's, accum[i] the skip destinations'; pool stays 0 (nothing is pooled: the gradient is computed at the low resolution).
TIED_ROUTES = ROUTES + ['mfma-11-masked', 'mfma-16-masked']      # octseg_conv_route with the values only octseg_tied_layer_route reports


def side_wgs():
    """Split-K width of the plan's weight gradients when they run on its side stream."""
    return L.lib().octseg_side_wgs()


def tied_dst_shape(layer, i):
    """Data gradient: the destination of source i -- the `up` source's at its stored (half) resolution."""
    s = layer.srcs[i]
    return (layer.N, layer.H >> s.up, layer.W >> s.up, s.C)


def tied_scratch_bytes(layer, dt=L.BF16):
    nb = L.lib().octseg_tied_layer_scratch_bytes(dt, C.byref(make_desc(layer, {}, 0)))
    if nb == 0:
        raise RuntimeError('octseg_tied_layer_scratch_bytes: ' + L.lib().octseg_last_error().decode())
    return nb


def tied_route_raw(mode, dt, desc, wg_target=0):
    r = (C.c_int * 8)()
    n = C.c_int(0)
    rc = L.lib().octseg_tied_layer_route(mode, dt, C.byref(desc), wg_target, r, C.byref(n))
    return rc, [r[i] for i in range(n.value)]


def tied_route(mode, layer, ptrs=None, wg_target=0, dt=L.BF16):
    """Kernel of every launch of the pass, as names (forward: skip, four parities; data gradient: up, skip; weight gradient: up launch(es), skip)."""
    ptrs = fake_ptrs(mode, layer) if ptrs is None else {'scratch': 0x400000, **ptrs}
    rc, r = tied_route_raw(mode, dt, make_desc(layer, ptrs, 1 << 40), wg_target)
    L.check(rc)
    names = WROUTES if mode == BACKWARD_WEIGHT else TIED_ROUTES
    return [None if v < 0 else names[v] for v in r]


def check_tied_tensors(mode, layer, t, T):
    """Every tensor of the call against the size the layer implies."""
    f32 = torch.float32
    assert set(t) == set(operand_names(mode, layer)), f'mode {mode} takes {operand_names(mode, layer)}, got {sorted(t)}'
    if mode != BACKWARD_DATA:
        for i, s in enumerate(layer.srcs):
            _need(t, f'x{i}', layer.src_shape(i), T)
            if s.affine:
                _need(t, f'scale{i}', (s.C,), f32)
                _need(t, f'shift{i}', (s.C,), f32)
    if mode != BACKWARD_WEIGHT:
        _need(t, 'w', layer.w_shape, f32)
    if mode == FORWARD:
        _need(t, 'y', (layer.N, layer.H, layer.W, layer.Cout), T)
    else:
        _need(t, 'dy', (layer.N, layer.H, layer.W, layer.Cout), T)
        if mode == BACKWARD_DATA:
            for i in range(len(layer.srcs)):
                _need(t, f'dx{i}', tied_dst_shape(layer, i), T)
        else:
            _need(t, 'dW', layer.w_shape, f32)


def tied_layer(mode, layer, t, wg_target=0, scratch=None):
    """Enqueue one pass of the tied `layer` on the current stream.  t: name -> device tensor (operand_names); returns the scratch (the packed
    images, and after a weight gradient the gradient of the 4x4 image: kept alive by the caller until the stream has run)."""
    t = {k: v for k, v in t.items() if v is not None}
    T = (t['dy'] if mode != FORWARD else t['x0']).dtype
    check_tied_tensors(mode, layer, t, T)
    ptrs = {k: v.data_ptr() for k, v in t.items()}
    nb = tied_scratch_bytes(layer, _DT[T])
    if scratch is None:
        scratch = torch.empty(nb, dtype=torch.uint8, device=t['dy' if mode != FORWARD else 'x0'].device)
    assert scratch.numel() >= nb and scratch.dtype == torch.uint8
    ptrs['scratch'] = scratch.data_ptr()
    L.check(L.lib().octseg_tied_layer_op(mode, _DT[T], C.byref(make_desc(layer, ptrs, nb)), wg_target, L.stream_ptr()))
    return scratch


# ------------------------------------------------------------------------------------------------ the stem kernels (csrc/stem_api.cpp)
STEM_IM2COL, STEM_FORWARD, STEM_WGRAD = 0, 1, 2
STEM_COUT, STEM_KP = 64, 160
STEM_KINDS = ((7, 3, 160), (3, 1, 32), (3, 0, 32))      # (ksize, pad, KP) of the im2col rows: ResNet, RegNet, EfficientNet


@dataclass
class Stem:
    """One stem launch over the NCHW f32 frame [N][3][H][W]; mean / std apply when `normalize`."""
    N: int
    H: int
    W: int
    normalize: bool = False
    mean: Tuple[float, ...] = (0.0, 0.0, 0.0)
    std: Tuple[float, ...] = (1.0, 1.0, 1.0)
    ksize: int = 7                 # IM2COL only
    pad: int = 3
    KP: int = 160
    relu_out: bool = False         # FORWARD only
    slab_row0: int = 0

    @property
    def img_shape(self):
        return (self.N, 3, self.H, self.W)

    @property
    def out_hw(self):
        return self.H // 2, self.W // 2

    @property
    def col_shape(self):
        return (self.N, self.H // 2, self.W // 2, self.KP)

    @property
    def y_shape(self):
        return (self.N, self.H // 2, self.W // 2, STEM_COUT)

    @property
    def w_shape(self):
        return (STEM_COUT, STEM_KP)


def stem_slab_rows(stem):
    return L.lib().octseg_stem_slab_rows(stem.N, stem.H, stem.W)


def make_stem_desc(stem, ptrs):
    """octseg_stem_desc of `stem`; ptrs: name -> device address (int) for img, col, w, wscale, bias, y, slab, dy, dW (absent = NULL)."""
    d = L.StemDesc()
    d.N, d.H, d.W, d.img, d.normalize = stem.N, stem.H, stem.W, ptrs.get('img'), int(stem.normalize)
    for i in range(3):
        d.mean[i], d.stdv[i] = stem.mean[i], stem.std[i]
    d.ksize, d.pad, d.KP, d.col = stem.ksize, stem.pad, stem.KP, ptrs.get('col')
    d.w, d.wscale, d.bias, d.relu_out = ptrs.get('w'), ptrs.get('wscale'), ptrs.get('bias'), int(stem.relu_out)
    d.y, d.stat_slab, d.slab_row0, d.dy, d.dW = ptrs.get('y'), ptrs.get('slab'), stem.slab_row0, ptrs.get('dy'), ptrs.get('dW')
    return d


def stem_operand_names(stage, has=()):
    """Names of the tensors a call of `stage` takes; `has`: which of wscale / bias / slab a forward carries."""
    if stage == STEM_IM2COL:
        return ['img', 'col']
    if stage == STEM_FORWARD:
        return ['img', 'w', 'y'] + [k for k in ('wscale', 'bias', 'slab') if k in has]
    return ['img', 'dy', 'dW']


def check_stem_tensors(stage, stem, t, T):
    """Every tensor of the call against the size the frame implies (the kernels trust these extents)."""
    f32 = torch.float32
    names = stem_operand_names(stage, has=tuple(t))
    assert set(t) == set(names), f'stage {stage} takes {names}, got {sorted(t)}'
    _need(t, 'img', stem.img_shape, f32)
    if stage == STEM_IM2COL:
        _need(t, 'col', stem.col_shape, T)
    elif stage == STEM_FORWARD:
        _need(t, 'w', stem.w_shape, f32)
        _need(t, 'y', stem.y_shape, T)
        for k in ('wscale', 'bias'):
            if k in t:
                _need(t, k, (STEM_COUT,), f32)
        if 'slab' in t:
            assert t['slab'].is_cuda and t['slab'].is_contiguous() and t['slab'].dtype == f32
            assert t['slab'].dim() == 3 and tuple(t['slab'].shape[1:]) == (STEM_COUT, 2)
            rows = stem_slab_rows(stem)
            assert t['slab'].shape[0] >= stem.slab_row0 + rows, f'slab: {t["slab"].shape[0]} rows, the launch writes [{stem.slab_row0}, {stem.slab_row0 + rows})'
    else:
        _need(t, 'dy', stem.y_shape, T)
        _need(t, 'dW', stem.w_shape, f32)


def stem(stage, stem_, t):
    """Enqueue one stem launch on the current stream.  t: name -> device tensor (stem_operand_names); the element type is that of col / y / dy."""
    t = {k: v for k, v in t.items() if v is not None}
    T = t[{STEM_IM2COL: 'col', STEM_FORWARD: 'y', STEM_WGRAD: 'dy'}[stage]].dtype
    check_stem_tensors(stage, stem_, t, T)
    ptrs = {k: v.data_ptr() for k, v in t.items()}
    L.check(L.lib().octseg_stem_op(stage, _DT[T], C.byref(make_stem_desc(stem_, ptrs)), L.stream_ptr()))
