"""Cases and reference of the single-launch tests of the tied decoder layer (tests/test_tiedops.py on the CPU, tests/test_gpu_tiedops.py on the GPU).

A case = one call of octseg_tied_layer_op (oct_segmentation_amd/convops.py: tied_layer): a conv_cases.Case whose layer is the (nearest x2, concat,
3x3 stride 1 pad 1) layer itself -- src 0 carries up = 1 -- plus the split-K width of a weight gradient.  `route` names every launch as
octseg_tied_layer_route reports it.

The reference of every pass is the PLAIN layer in float64 (conv_ref.forward_f32value / backward_data_full / backward_weight of that Layer): the nine
taps over the upsampled concatenation, never the 4x4 image -- a wrong decomposition cannot hide behind a matching reference.  Only the store
rules are the tied path's own (csrc/kernels.h):
  forward        Cs > 0: the skip slice's launch stores T(s), the parity launch that owns the pixel adds T(u): y = T(f32(T(u)) + T(s)), u / s = the
                 layer's sum over the up / skip channels; Cs = 0: y = T(u)
  data gradient  low resolution: T(g), accumulated T(f32(T(g)) + old), g = the WHOLE sum over the 2x2 quad and all taps (the plain path's pooled
                 rule T(old + T(q00) + ..) does not apply); skip sources: the 'staged' rule of conv_ref.store
  weight gradient  old dW + the plain layer's gradient (the fold adds f32 sums onto what dW held)
Judged as the conv cases are: exact operands (conv_cases: weights in {0, +-0.25, +-0.5, +-1}, so every 4x4 entry -- a sum of at most four taps -- is a
bf16) bit for bit; Gaussian operands by Rule R.  The Gaussian weights are multiples of 2^-5 below 1, so every sum of four taps is a bf16
too (at most 7 significant bits): the 4x4 image as the kernel sees it is the exact sum, T(float64 sum), without ambiguity, and the plain
reference stays the reference.  Rule R's n is the number of products the plain layer adds per output (>= the tied path's, whose products
are sums of the plain ones: sum |terms| of the plain layer bounds the tied one's by the triangle inequality).
"""
from dataclasses import dataclass

import torch

import conv_cases as CC
import conv_ref as CR
from conv_cases import AR, DENSE, DGRAD, FWD, WGRAD, A, P
from oct_segmentation_amd import convops as CO
from oct_segmentation_amd.convops import Layer

BF16 = torch.bfloat16


@dataclass
class Tied:
    case: CC.Case
    wg_target: int = 0          # weight gradient: 0 = the full split-K width, SIDE = the plan's side-stream narrowing

    @property
    def id(self):
        return self.case.id + (f'.wg{self.wg_target}' if self.wg_target else '')


def up(C, kind=P):
    s = kind(C)
    s.up = 1
    return s


def _layer(N, h, w, Cout, srcs, accum=(0, 0, 0, 0, 0)):
    """h x w: the LOW resolution (the stored extent of src 0)."""
    return Layer(N, 2 * h, 2 * w, 3, Cout, srcs, pad=1, accum=tuple(accum))


M16, M11, U16 = 'mfma-16-masked', 'mfma-11-masked', 'mfma-16'


def shapes():
    """name -> (layer maker(accum), data-gradient routes (up, skip))."""
    return {
        # masked 8x16 tile: ragged tiles (12 x 20), partial N tile (72 of 128), planes of one K chunk (Cout 64)
        'm16_cs0': (lambda acc=(0,) * 5: _layer(2, 12, 20, 64, [up(72, AR)], acc), (M16,)),
        'm16_cs32': (lambda acc=(0,) * 5: _layer(2, 12, 20, 64, [up(72, AR), A(32)], acc), (M16, 'mfma-16')),
        # masked 11x11 tile: two K chunks per plane (Cout 128), second N tile 8 channels wide (136)
        'm11': (lambda acc=(0,) * 5: _layer(2, 11, 22, 128, [up(136, AR), P(40)], acc), (M11, 'mfma-16')),
        # the 16-tap stride-2 fallback: planes that are no whole chunks (Cout 32)
        'u32': (lambda acc=(0,) * 5: _layer(3, 6, 10, 32, [up(64, AR), P(32)], acc), (U16, 'mfma-16')),
        # ... and a masked launch whose own Cout (= Ca) is not above 64
        'u64': (lambda acc=(0,) * 5: _layer(3, 6, 10, 64, [up(64, P)], acc), (U16,)),
        # one tile of wgrad_convt.hip: below wgrad_convt16_eligible's two workgroups, so the four parity launches of wgrad_mfma
        'w1tile': (lambda acc=(0,) * 5: _layer(1, 4, 8, 64, [up(64, AR), P(32)], acc), (U16, 'mfma-16')),
        # several skips: c0 offsets of the skip slice, store / add per destination
        'skips2': (lambda acc=(0,) * 5: _layer(2, 12, 20, 64, [up(72, P), AR(32), P(40)], acc), (M16, 'mfma-16')),
    }


def _case(name, mode, layer, route, nnz=None, exact=True):
    c = CC.Case(name, mode, BF16, layer, tuple(route), (), exact, nnz)
    c.group = 'tied'
    return c


def side():
    return CO.side_wgs()


def forward_routes(layer):
    return (('mfma-16',) if len(layer.srcs) > 1 else ()) + ('mfma-16',) * 4


def make_cases(wroutes):
    """wroutes: name -> weight-gradient routes of the shape (asked from octseg_tied_layer_route once: test_tiedops.py pins them)."""
    S = shapes()
    out = []
    for name, (mk, droute) in S.items():
        Ly = mk()
        half = 9 * Ly.Cin // 2
        out.append(Tied(_case(name, FWD, Ly, forward_routes(Ly), nnz=half)))
        out.append(Tied(_case(name, DGRAD, Ly, droute)))
        out.append(Tied(_case(name, WGRAD, Ly, wroutes[name])))
    # values that leave bf16's 8 bits: the store rules can be told apart
    for name in ('m16_cs32', 'm11', 'u32'):
        mk, droute = S[name]
        out.append(Tied(_case(name + '_dense', FWD, mk(), forward_routes(mk()), nnz=DENSE)))
        out.append(Tied(_case(name + '_dense_acc', DGRAD, mk((1, 1, 0, 0, 0)), droute, nnz=DENSE)))
    out.append(Tied(_case('m16_cs0_dense_acc', DGRAD, S['m16_cs0'][0]((1, 0, 0, 0, 0)), S['m16_cs0'][1], nnz=DENSE)))
    out.append(Tied(_case('skips2_acc001', DGRAD, S['skips2'][0]((0, 0, 1, 0, 0)), S['skips2'][1], nnz=DENSE)))
    out.append(Tied(_case('skips2_acc101', DGRAD, S['skips2'][0]((1, 0, 1, 0, 0)), S['skips2'][1], nnz=DENSE)))
    # both split-K widths on each side of wgrad_convt16_eligible
    for name in ('m16_cs32', 'u32', 'm11', 'w1tile'):
        out.append(Tied(_case(name, WGRAD, S[name][0](), wroutes[name]), wg_target=side()))
    # Gaussian operands
    out.append(Tied(_case('m16_cs0_gauss', FWD, S['m16_cs0'][0](), forward_routes(S['m16_cs0'][0]()), exact=False)))
    for name in ('m16_cs32', 'm11', 'u32'):
        out.append(Tied(_case(name + '_gauss', DGRAD, S[name][0](), S[name][1], exact=False)))
        out.append(Tied(_case(name + '_gauss', WGRAD, S[name][0](), wroutes[name], exact=False)))
    out.append(Tied(_case('m11_gauss', WGRAD, S['m11'][0](), wroutes['m11'], exact=False), wg_target=side()))
    out.append(Tied(_case('w1tile_gauss', WGRAD, S['w1tile'][0](), wroutes['w1tile'], exact=False)))
    return out


def query_wroutes():
    return {name: tuple(CO.tied_route(WGRAD, mk())) for name, (mk, _) in shapes().items()}


def all_cases():
    return make_cases(query_wroutes())


# ------------------------------------------------------------------------------------------------ operands
def gaussian_weights(shape, g):
    """Multiples of 2^-5 in (-1, 1): bf16 values whose sums of up to four are bf16 values too."""
    w = (torch.randn(shape, generator=g, dtype=torch.float64) * 0.25 * 32).round().clamp(-31, 31) / 32
    return w.to(torch.float32)


def make_operands(tc):
    case = tc.case
    t = CC.make_operands(case)
    g = torch.Generator().manual_seed(CC.zlib.crc32((tc.id + '.tied').encode()))
    Ly = case.layer
    if case.mode == DGRAD:      # the `up` source's gradient lives at its stored resolution
        ds = CO.tied_dst_shape(Ly, 0)
        t['dx0'] = torch.randint(-4, 5, ds, generator=g).to(BF16) if Ly.accum[0] else torch.full(ds, float('nan'), dtype=BF16)
    if not case.exact and 'w' in t:
        t['w'] = gaussian_weights(Ly.w_shape, g)
    return t


# ------------------------------------------------------------------------------------------------ reference
def split(layer):
    """(Ca, Cs)."""
    return layer.srcs[0].C, layer.Cin - layer.srcs[0].C


def forward_parts(layer, t, T):
    """(u, s): the plain layer's sum over the up / skip channels, [N][Cout][H][W] each (s is None without skips)."""
    Ca, Cs = split(layer)
    xp, w = CR.virtual_input(layer, t, T), CR.weight_as_seen(layer, t, T)
    u = CR.conv_of(layer, xp[:, :Ca], w[..., :Ca])
    s = CR.conv_of(layer, xp[:, Ca:], w[..., Ca:]) if Cs else None
    return u, s


def forward(layer, t, T, rule='tied'):
    u, s = forward_parts(layer, t, T)
    if s is None:
        return {'y': CR.nhwc(CR.rnd(u, T))}
    if rule == 'whole':          # a deliberately wrong rule: the sum rounded once
        return {'y': CR.nhwc(CR.rnd(u + s, T))}
    return {'y': CR.nhwc(CR.rnd(CR.rnd(u, T) + CR.rnd(s, T), T))}


def backward_data_values(layer, t, T):
    """(low-resolution f32 value of the up source's gradient [N][Ca][H/2][W/2], the plain layer's full gradient [N][Cin][H][W])."""
    Ca, _ = split(layer)
    g = CR.backward_data_full(layer, t, T)
    gu = g[:, :Ca]
    low = gu[:, :, 0::2, 0::2] + gu[:, :, 0::2, 1::2] + gu[:, :, 1::2, 0::2] + gu[:, :, 1::2, 1::2]
    return low, g


def backward_data(layer, t, T, rule='tied'):
    low, g = backward_data_values(layer, t, T)
    Ca, _ = split(layer)
    out = {}
    if rule == 'pooled':         # the plain path's pooled rule (conv_ref.pool_store, 'staged'): a deliberately wrong rule here
        old = CR.nchw(CR.ref(t['dx0'])) if layer.accum[0] else None
        out['dx0'] = CR.nhwc(CR.pool_store(g[:, :Ca], old, T, layer.accum[0], 'staged'))
    else:
        old = CR.nchw(CR.ref(t['dx0'])) if layer.accum[0] else None
        out['dx0'] = CR.nhwc(CR.store(low, old, T, layer.accum[0], 'staged'))
    c0 = Ca
    for i, s in enumerate(layer.srcs[1:], start=1):
        old = CR.nchw(CR.ref(t[f'dx{i}'])) if layer.accum[i] else None
        out[f'dx{i}'] = CR.nhwc(CR.store(g[:, c0:c0 + s.C], old, T, layer.accum[i], 'staged'))
        c0 += s.C
    return out


def backward_weight(layer, t, T):
    return CR.backward_weight(layer, t, T)


def reference(tc, t, rule='tied'):
    c = tc.case
    if c.mode == FWD:
        return forward(c.layer, t, c.T, rule)
    if c.mode == DGRAD:
        return backward_data(c.layer, t, c.T, rule)
    return backward_weight(c.layer, t, c.T)
