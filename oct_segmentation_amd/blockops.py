"""Single-stage bindings of the PAN feature-pyramid-attention kernels (csrc/pan.hip) and the MAnet position-attention kernels
(csrc/pab.hip) over ``octseg_fpa_op`` / ``octseg_pab_op`` (csrc/block_api.cpp, include/octseg.h).

Like ``sweeps.py`` and ``convops.py`` they exist so that each HIP kernel can be pinned against a float64 reference alone
(tests/test_gpu_blockops.py); the network path reaches the same launchers through the plan.  One call is one launcher.  Every wrapper
derives the extent of every buffer from the shapes and checks the tensors against it before the call; the library checks alignment,
vector widths, dtypes, null pointers, scratch sizes and GEMM reach and refuses with a status (``fpa_op_raw`` / ``pab_op_raw`` return it).

The pyramid keeps every intermediate in one float scratch: ``fpa_scratch_views`` / ``fpa_gscratch_views`` name its pieces.  The six
``pab_gemm`` call sites of plan_forward.cpp / plan_backward.cpp are restated as named constructors (``gemm_S`` ... ``gemm_dtop``).
"""
import ctypes as C
from dataclasses import dataclass

import torch

from . import _lib as L
from .ops import _dt

FPA_STAGES = ('maxpool2_fwd', 'maxpool2_bwd', 'in_fwd', 'in_bwd', 'pyr_fwd', 'pyr_bwd', 'mix_fwd', 'mix_bwd')      # octseg_fpa_stage
PAB_STAGES = ('gemm', 'softmax_fwd', 'softmax_bwd', 'mix_fwd', 'mix_bwd')                                          # octseg_pab_stage
FPA = {n: i for i, n in enumerate(FPA_STAGES)}
PAB = {n: i for i, n in enumerate(PAB_STAGES)}
PYR_K = (7, 5, 3, 3, 5, 7)      # conv size of layers 0..5 = down1, down2, down3.1, down3.2, conv2, conv1
PAB_CHANNELS = 64               # center / top: 1x1 convs to 64 channels


def fpa_op_raw(stage, dtype, desc, stream=None):
    return L.lib().octseg_fpa_op(FPA[stage] if isinstance(stage, str) else stage, dtype, None if desc is None else C.byref(desc), stream)


def pab_op_raw(stage, dtype, desc, stream=None):
    return L.lib().octseg_pab_op(PAB[stage] if isinstance(stage, str) else stage, dtype, None if desc is None else C.byref(desc), stream)


def _need(t, numel, dtype, what):
    assert t is not None, f'{what} is required'
    assert t.is_contiguous(), f'{what}: a contiguous tensor is expected'
    assert t.dtype == dtype, f'{what}: {t.dtype}, expected {dtype}'
    assert t.numel() == numel, f'{what}: {t.numel()} elements, expected {numel}'


def _f32(t, numel, what):
    _need(t, numel, torch.float32, what)


def _go(fn, stage, dtype, desc, tensors):
    for t in tensors:
        assert t is None or t.is_cuda, f'{stage}: device tensors expected'
    L.check(fn(stage, dtype, desc, L.stream_ptr()))


# ---------------------------------------------------------------- the pyramid's scratch layouts (pan.hip)
def fpa_levels(N, h, w):
    """(h, w) of the block's map and of pyramid levels 1..3, and their element counts n0..n3."""
    assert N >= 1 and h // 8 >= 1 and w // 8 >= 1, 'the pyramid needs h / 8 >= 1 and w / 8 >= 1'
    dims = [(h, w), (h // 2, w // 2), (h // 2 // 2, w // 2 // 2), (h // 2 // 2 // 2, w // 2 // 2 // 2)]
    return dims, [N * a * b for a, b in dims]


def fpa_scratch_floats(N, h, w):
    _, (n0, n1, n2, n3) = fpa_levels(N, h, w)
    return 5 * n1 + 7 * n2 + 5 * n3 + n0 + 16


def fpa_gscratch_floats(N, h, w):
    _, (n0, n1, n2, n3) = fpa_levels(N, h, w)
    return 3 * n1 + 4 * n2 + 3 * n3


def fpa_uu_offset(N, h, w):
    return fpa_scratch_floats(N, h, w) - 16 - N * h * w


def _views(layout, scratch):
    out, off = {}, 0
    for name, shape in layout:
        n = 1
        for s in shape:
            n *= s
        out[name] = (off, shape) if scratch is None else scratch[off:off + n].view(*shape)
        off += n
    return out, off


def fpa_scratch_views(N, h, w, scratch=None):
    """name -> (offset in floats, shape), or -> view of `scratch` (float32, at least fpa_scratch_floats): the forward's intermediates.
    Level 1: r1 (x1raw, the caller's input), x1, c1 (conv1 raw), y1, tu (up(t) + y1 = u);  level 2: p2, r2, x2, c2, y2, x3u, t;
    level 3: p3, r3a, x3a, r3b, x3;  uu [N, h, w];  stats: 6 x (mean, rstd) in layer order (4 more floats are spare)."""
    dims, _ = fpa_levels(N, h, w)
    lay = [(k, (N,) + dims[1]) for k in ('r1', 'x1', 'c1', 'y1', 'tu')] + [(k, (N,) + dims[2]) for k in ('p2', 'r2', 'x2', 'c2', 'y2', 'x3u', 't')] + \
          [(k, (N,) + dims[3]) for k in ('p3', 'r3a', 'x3a', 'r3b', 'x3')] + [('uu', (N,) + dims[0]), ('stats', (12,)), ('spare', (4,))]
    if scratch is not None:
        _f32(scratch, fpa_scratch_floats(N, h, w), 'scratch')
    v, off = _views(lay, scratch)
    assert off == fpa_scratch_floats(N, h, w) and (scratch is not None or v['uu'][0] == fpa_uu_offset(N, h, w))
    return v


def fpa_gscratch_views(N, h, w, gscratch=None):
    """The gradient scratch: du, dx1 (d x1raw when the kernel ends: what fpa_in_bwd reads at gscratch + n1), dy1; dt, dx2, dy2, dp2; dx3, dx3a, dp3."""
    dims, _ = fpa_levels(N, h, w)
    lay = [(k, (N,) + dims[1]) for k in ('du', 'dx1', 'dy1')] + [(k, (N,) + dims[2]) for k in ('dt', 'dx2', 'dy2', 'dp2')] + \
          [(k, (N,) + dims[3]) for k in ('dx3', 'dx3a', 'dp3')]
    if gscratch is not None:
        _f32(gscratch, fpa_gscratch_floats(N, h, w), 'gscratch')
    v, off = _views(lay, gscratch)
    assert off == fpa_gscratch_floats(N, h, w)
    return v


# ---------------------------------------------------------------- pan.hip
def maxpool2_fwd(x, p):
    N, H, W, Cn = x.shape
    _need(x, N * H * W * Cn, x.dtype, 'x')
    _need(p, N * (H // 2) * (W // 2) * Cn, x.dtype, 'p')
    d = L.FpaDesc(N=N, H=H, W=W, C=Cn, x=x.data_ptr(), p=p.data_ptr())
    _go(fpa_op_raw, 'maxpool2_fwd', _dt(x), d, (x, p))


def maxpool2_bwd(x, dp, dx, accum):
    N, H, W, Cn = x.shape
    _need(x, N * H * W * Cn, x.dtype, 'x')
    _need(dp, N * (H // 2) * (W // 2) * Cn, x.dtype, 'dp')
    _need(dx, N * H * W * Cn, x.dtype, 'dx')
    d = L.FpaDesc(N=N, H=H, W=W, C=Cn, accum=int(accum), x=x.data_ptr(), dp=dp.data_ptr(), dx=dx.data_ptr())
    _go(fpa_op_raw, 'maxpool2_bwd', _dt(x), d, (x, dp, dx))


def fpa_in_fwd(p, w, b, y, K=7):
    N, H, W, Cn = p.shape
    _need(p, N * H * W * Cn, p.dtype, 'p')
    _f32(w, K * K * Cn, 'w')
    _f32(b, 1, 'b')
    _f32(y, N * H * W, 'y')
    d = L.FpaDesc(N=N, H=H, W=W, C=Cn, K=K, p=p.data_ptr(), w=w.data_ptr(), b=b.data_ptr(), y=y.data_ptr())
    _go(fpa_op_raw, 'in_fwd', _dt(p), d, (p, w, b, y))


def fpa_in_bwd(p, dy, w, dp, dw, db, K=7):
    N, H, W, Cn = p.shape
    _need(p, N * H * W * Cn, p.dtype, 'p')
    _need(dp, N * H * W * Cn, p.dtype, 'dp')
    _f32(dy, N * H * W, 'dy')
    _f32(w, K * K * Cn, 'w')
    _f32(dw, K * K * Cn, 'dw')
    _f32(db, 1, 'db')
    d = L.FpaDesc(N=N, H=H, W=W, C=Cn, K=K, p=p.data_ptr(), dy=dy.data_ptr(), w=w.data_ptr(), dp=dp.data_ptr(), dw=dw.data_ptr(), db=db.data_ptr())
    _go(fpa_op_raw, 'in_bwd', _dt(p), d, (p, dy, w, dp, dw, db))


def _pyr_desc(N, h, w, prm, fields, conv_fields):
    """prm: name -> list of 6 float32 tensors (layer 0 of the conv fields may be None: its conv is fpa_in_*)."""
    d = L.FpaDesc(N=N, H=h, W=w)
    ts = []
    for f, key in fields + conv_fields:
        assert len(prm[key]) == 6, f'{key}: six layers'
        arr = getattr(d, f)
        for l in range(6):
            t = prm[key][l]
            if (f, key) in conv_fields:
                if l == 0 and t is None:
                    continue
                _f32(t, 1 if key in ('b', 'db') else PYR_K[l] ** 2, f'{key}[{l}]')
            else:
                _f32(t, 1, f'{key}[{l}]')
            arr[l] = t.data_ptr()
            ts.append(t)
    return d, ts


def fpa_pyr_fwd(scratch, prm, N, h, w, train, dtype=L.F32):
    """scratch[0 .. n1) holds x1raw; prm: w, b, gamma, beta, rm, rv (lists of 6)."""
    _f32(scratch, fpa_scratch_floats(N, h, w), 'scratch')
    d, ts = _pyr_desc(N, h, w, prm, [('pg', 'gamma'), ('pbe', 'beta'), ('prm', 'rm'), ('prv', 'rv')], [('pw', 'w'), ('pb', 'b')])
    d.train, d.scratch, d.scratch_floats = int(train), scratch.data_ptr(), scratch.numel()
    _go(fpa_op_raw, 'pyr_fwd', dtype, d, ts + [scratch])


def fpa_pyr_bwd(scratch, gscratch, duu, prm, N, h, w, dtype=L.F32):
    """After fpa_pyr_fwd(train = 1) on the same scratch; prm: w, gamma, dw, db, dgamma, dbeta (lists of 6)."""
    _f32(scratch, fpa_scratch_floats(N, h, w), 'scratch')
    _f32(gscratch, fpa_gscratch_floats(N, h, w), 'gscratch')
    _f32(duu, N * h * w, 'duu')
    d, ts = _pyr_desc(N, h, w, prm, [('pg', 'gamma'), ('pdg', 'dgamma'), ('pdbe', 'dbeta')], [('pw', 'w'), ('pdw', 'dw'), ('pdb', 'db')])
    d.scratch, d.scratch_floats, d.gscratch, d.gscratch_floats, d.duu = scratch.data_ptr(), scratch.numel(), gscratch.data_ptr(), gscratch.numel(), duu.data_ptr()
    _go(fpa_op_raw, 'pyr_bwd', dtype, d, ts + [scratch, gscratch, duu])


def fpa_mix_fwd(uu, mid, b1, out):
    N, HW, Cn = mid.shape
    _f32(uu, N * HW, 'uu')
    _need(mid, N * HW * Cn, mid.dtype, 'mid')
    _need(b1, N * Cn, mid.dtype, 'b1')
    _need(out, N * HW * Cn, mid.dtype, 'out')
    d = L.FpaDesc(N=N, H=HW, W=1, C=Cn, uu=uu.data_ptr(), mid=mid.data_ptr(), b1=b1.data_ptr(), out=out.data_ptr())
    _go(fpa_op_raw, 'mix_fwd', _dt(mid), d, (uu, mid, b1, out))


def fpa_mix_bwd(uu, mid, g, dmid, duu):
    N, HW, Cn = mid.shape
    _f32(uu, N * HW, 'uu')
    _f32(duu, N * HW, 'duu')
    for n, t in (('mid', mid), ('g', g), ('dmid', dmid)):
        _need(t, N * HW * Cn, mid.dtype, n)
    d = L.FpaDesc(N=N, H=HW, W=1, C=Cn, uu=uu.data_ptr(), mid=mid.data_ptr(), g=g.data_ptr(), dmid=dmid.data_ptr(), duu=duu.data_ptr())
    _go(fpa_op_raw, 'mix_bwd', _dt(mid), d, (uu, mid, g, dmid, duu))


# ---------------------------------------------------------------- pab.hip
@dataclass
class Gemm:
    """One pab_gemm call site: C[b][m][n] (+)= sum_k A[b][m][k] B[b][k][n].  s*: (batch, row, column) strides in elements; *_f32: the operand
    is float32 scratch (else of the tensor dtype); numel*: elements per image of the three buffers."""
    name: str
    M: int
    N: int
    K: int
    sA: tuple
    sB: tuple
    sC: tuple
    a_f32: int
    b_f32: int
    c_f32: int
    numelA: int
    numelB: int
    numelC: int


# the stride sets of plan_forward.cpp (OP_PAB) and plan_backward.cpp (OP_PAB), restated; hw pixels, Cn channels, Kc = 64
def gemm_S(hw, Cn, Kc=PAB_CHANNELS):        # S[i][j] = sum_k center[i][k] top[j][k]
    return Gemm('S', hw, hw, Kc, (hw * Kc, Kc, 1), (hw * Kc, 1, Kc), (hw * hw, hw, 1), 0, 0, 1, hw * Kc, hw * Kc, hw * hw)


def gemm_M(hw, Cn, Kc=PAB_CHANNELS):        # M[i][c] = sum_j P[i][j] bottom[j][c]
    return Gemm('M', hw, Cn, hw, (hw * hw, hw, 1), (hw * Cn, Cn, 1), (hw * Cn, Cn, 1), 1, 0, 1, hw * hw, hw * Cn, hw * Cn)


def gemm_dP(hw, Cn, Kc=PAB_CHANNELS):       # dP[i][j] = sum_c dM[i][c] bottom[j][c]
    return Gemm('dP', hw, hw, Cn, (hw * Cn, Cn, 1), (hw * Cn, 1, Cn), (hw * hw, hw, 1), 1, 0, 1, hw * Cn, hw * Cn, hw * hw)


def gemm_dbottom(hw, Cn, Kc=PAB_CHANNELS):  # dbottom[j][c] = sum_i P[i][j] dM[i][c]
    return Gemm('dbottom', hw, Cn, hw, (hw * hw, 1, hw), (hw * Cn, Cn, 1), (hw * Cn, Cn, 1), 1, 1, 0, hw * hw, hw * Cn, hw * Cn)


def gemm_dcenter(hw, Cn, Kc=PAB_CHANNELS):  # dcenter[i][k] = sum_j dS[i][j] top[j][k]
    return Gemm('dcenter', hw, Kc, hw, (hw * hw, hw, 1), (hw * Kc, Kc, 1), (hw * Kc, Kc, 1), 1, 0, 0, hw * hw, hw * Kc, hw * Kc)


def gemm_dtop(hw, Cn, Kc=PAB_CHANNELS):     # dtop[j][k] = sum_i dS[i][j] center[i][k]
    return Gemm('dtop', hw, Kc, hw, (hw * hw, 1, hw), (hw * Kc, Kc, 1), (hw * Kc, Kc, 1), 1, 0, 0, hw * hw, hw * Kc, hw * Kc)


GEMMS = {f.__name__[5:]: f for f in (gemm_S, gemm_M, gemm_dP, gemm_dbottom, gemm_dcenter, gemm_dtop)}


def gemm_desc(g, batch, A, B, Cm, accum=0, numel=None):
    """octseg_pab_desc of call site g; A, B, Cm: device addresses (int)."""
    d = L.PabDesc()
    s = d.gemm
    s.A, s.B, s.C = A, B, Cm
    (s.sAb, s.sAm, s.sAk), (s.sBb, s.sBk, s.sBn), (s.sCb, s.sCm, s.sCn) = g.sA, g.sB, g.sC
    s.M, s.N, s.K, s.batch, s.a_f32, s.b_f32, s.c_f32, s.accum = g.M, g.N, g.K, batch, g.a_f32, g.b_f32, g.c_f32, int(accum)
    d.numelA, d.numelB, d.numelC = numel if numel is not None else (batch * g.numelA, batch * g.numelB, batch * g.numelC)
    return d


def pab_gemm(g, A, B, Cm, batch, accum=0, dtype=None):
    """dtype: the tensor dtype T of the call (default: that of the first operand that is not float32 scratch)."""
    T = None
    for t, f32 in ((A, g.a_f32), (B, g.b_f32), (Cm, g.c_f32)):
        if not f32:
            T = t.dtype if T is None else T
            assert t.dtype == T, f'gemm {g.name}: operands of one tensor dtype expected'
    if dtype is None:
        assert T is not None, f'gemm {g.name}: every operand is float32 scratch: pass dtype'
        dtype = {torch.float32: L.F32, torch.bfloat16: L.BF16, torch.float16: L.F16}[T]
    T = {L.F32: torch.float32, L.BF16: torch.bfloat16, L.F16: torch.float16}[dtype]
    for n, t, f32, numel in (('A', A, g.a_f32, g.numelA), ('B', B, g.b_f32, g.numelB), ('C', Cm, g.c_f32, g.numelC)):
        _need(t, batch * numel, torch.float32 if f32 else T, f'gemm {g.name} {n}')
    _go(pab_op_raw, 'gemm', dtype, gemm_desc(g, batch, A.data_ptr(), B.data_ptr(), Cm.data_ptr(), accum), (A, B, Cm))


def pab_softmax_fwd(S, dtype=L.F32):
    """S [batch, n] float32: softmax over all n entries of each image, in place."""
    batch, n = S.shape
    _f32(S, batch * n, 'S')
    d = L.PabDesc(S=S.data_ptr(), batch=batch, n=n)
    _go(pab_op_raw, 'softmax_fwd', dtype, d, (S,))


def pab_softmax_bwd(dP, P, dtype=L.F32):
    """dP [batch, n] -> P (dP - sum P dP) in place; P is only read."""
    batch, n = P.shape
    _f32(P, batch * n, 'P')
    _f32(dP, batch * n, 'dP')
    d = L.PabDesc(S=dP.data_ptr(), P=P.data_ptr(), batch=batch, n=n)
    _go(pab_op_raw, 'softmax_bwd', dtype, d, (dP, P))


def pab_mix_fwd(x, M, y):
    N, HW, Cn = x.shape
    _need(x, N * HW * Cn, x.dtype, 'x')
    _need(y, N * HW * Cn, x.dtype, 'y')
    _f32(M, N * HW * Cn, 'M')
    d = L.PabDesc(x=x.data_ptr(), M=M.data_ptr(), y=y.data_ptr(), N=N, HW=HW, C=Cn)
    _go(pab_op_raw, 'mix_fwd', _dt(x), d, (x, M, y))


def pab_mix_bwd(dy, dM):
    N, HW, Cn = dy.shape
    _need(dy, N * HW * Cn, dy.dtype, 'dy')
    _f32(dM, N * HW * Cn, 'dM')
    d = L.PabDesc(dy=dy.data_ptr(), dM=dM.data_ptr(), N=N, HW=HW, C=Cn)
    _go(pab_op_raw, 'mix_bwd', _dt(dy), d, (dy, dM))
