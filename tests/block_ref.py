"""float64 references of the PAN pyramid kernels (csrc/pan.hip) and the MAnet position-attention kernels (csrc/pab.hip).

Plain torch restatements of one launcher -- or, for the one-workgroup pyramid, of one of its ~20 phases -- on the kernels' own
layouts (NHWC tensors, one-channel [N, H, W] maps, flat strided GEMM operands), evaluated in float64 (sweep_ref.REF_DTYPE) on
inputs first rounded to the tested dtype.  The comparison rules X / E / R / T, the guarded buffers and the input generators are
sweep_ref's.  tests/test_blockops.py checks these references against torch.nn.functional / autograd (CPU, NCHW, float64);
tests/test_gpu_blockops.py checks the kernels against them.

Bilinear coordinates and weights are formed in float32 exactly as pan.hip's pyr_bil_coord forms them (sc = (float)(in - 1) /
(float)(out - 1), f = sc * o, i0 = (int)f, l = f - i0); the arithmetic on them is float64.
"""
import torch
import torch.nn.functional as F

import sweep_ref as R
from sweep_ref import d

PYR_K = (7, 5, 3, 3, 5, 7)
BN_EPS, BN_MOM = 1e-5, 0.1


def _rd():
    return R.REF_DTYPE[0]


# ------------------------------------------------------------------------------------------------ maxpool2 (NHWC vectors)
def _quads(x):
    """[N, H, W, C] -> [4, N, H/2, W/2, C] in scan order k = 2 dy + dx."""
    return torch.stack([x[:, 0::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 0::2], x[:, 1::2, 1::2]])


def maxpool2_fwd(x):
    return _quads(d(x)).max(0).values


def maxpool2_argmax(x):
    """Index (0..3, scan order) of the FIRST maximum of every window."""
    q = _quads(d(x))
    is_max = q == q.max(0).values
    code = (is_max.to(torch.int64) * torch.tensor([8, 4, 2, 1]).view(4, 1, 1, 1, 1)).sum(0)      # the first maximum is the highest bit
    return 3 - code.clamp_min(1).to(torch.float64).log2().floor().to(torch.int64)


def maxpool2_bwd(x, dp, dx0=None):
    """dx: dp to the first maximum of its window, 0 to the three others; dx0: accumulated onto."""
    x, dp = d(x), d(dp)
    am = maxpool2_argmax(x)
    out = torch.zeros_like(x)
    for k, (dy, dx_) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        out[:, dy::2, dx_::2] = torch.where(am == k, dp, torch.zeros_like(dp))
    return out if dx0 is None else out + d(dx0)


# ------------------------------------------------------------------------------------------------ the wide K x K conv to one channel
def _shifted(p, K):
    """Yields (t, window) with window[n, y, x, ...] = p[n, y + t / K - K / 2, x + t % K - K / 2, ...] (zero outside)."""
    pad = K // 2
    H, W = p.shape[1], p.shape[2]
    pp = torch.zeros((p.shape[0], H + 2 * pad, W + 2 * pad) + tuple(p.shape[3:]), dtype=p.dtype)
    pp[:, pad:pad + H, pad:pad + W] = p
    for t in range(K * K):
        r, s = t // K, t % K
        yield t, pp[:, r:r + H, s:s + W]


def fpa_in_fwd(p, w, b, K):
    """-> y [N, H, W], sum|terms| (bias included)."""
    p, w, b = d(p), d(w).view(K * K, -1), d(b)
    y = torch.zeros(p.shape[:3], dtype=_rd()) + b
    sa = torch.zeros(p.shape[:3], dtype=_rd()) + b.abs()
    for t, win in _shifted(p, K):
        y = y + (win * w[t]).sum(-1)
        sa = sa + (win * w[t]).abs().sum(-1)
    return y, sa


def fpa_in_bwd(p, dy, w, dw0, db0, K):
    """-> dict ref, sumabs of dp [N, H, W, C], dw [K K, C], db [1]."""
    p, dy, w, dw0, db0 = d(p), d(dy), d(w).view(K * K, -1), d(dw0).view(K * K, -1), d(db0)
    dp = torch.zeros_like(p)
    dpa = torch.zeros_like(p)
    dw = dw0.clone()
    dwa = dw0.abs()
    flipped = dict(_shifted(dy, K))       # window[n, y, x] = dy[n, y + r - K/2, x + s - K/2]
    for t, win in _shifted(p, K):
        # dp[n, y, x, c] += w[t, c] dy[n, y - r + K/2, x - s + K/2]: the window of the mirrored tap
        g = flipped[K * K - 1 - t]
        dp = dp + g.unsqueeze(-1) * w[t]
        dpa = dpa + (g.unsqueeze(-1) * w[t]).abs()
        dw[t] = dw[t] + (dy.unsqueeze(-1) * win).sum((0, 1, 2))
        dwa[t] = dwa[t] + (dy.unsqueeze(-1) * win).abs().sum((0, 1, 2))
    return dict(dp=(dp, dpa), dw=(dw, dwa), db=(db0 + dy.sum(), db0.abs() + dy.abs().sum()))


# ------------------------------------------------------------------------------------------------ the pyramid's phases (one-channel maps [N, H, W])
def pyr_conv(x, w, b, K):
    """-> ref, sum|terms|; n = K K + 1 terms."""
    y, sa = fpa_in_fwd(d(x).unsqueeze(-1), d(w).view(K * K, 1), d(b).view(1), K)
    return y, sa


def pyr_bn_stats(raw):
    """Batch statistics of one channel: mean, biased var, unbiased var, sum|raw| / n (float64 scalars)."""
    r = d(raw).reshape(-1)
    n = r.numel()
    mean = r.mean()
    ssd = ((r - mean) ** 2).sum()
    return mean, ssd / n, (ssd / (n - 1) if n > 1 else ssd / n), r.abs().mean()


BN_OUT_K = 4 + 2        # (raw - mean), * rstd, * gamma, + beta
BN_EVAL_K = 4 + 3 + 2   # + rvar + eps, sqrtf, 1 / . of the eval path's own rstd
RUN_K = 4 + 2           # 0.9 r, 0.1 v, +, and the rounding of v to float


def pyr_bn_relu_out(raw, mean, rstd, gamma, beta):
    """relu((raw - mean) rstd gamma + beta) with the GIVEN mean / rstd (the kernel's own: teacher-forced) -> z, relu(z), mag."""
    raw, mean, rstd, gamma, beta = d(raw), d(mean), d(rstd), d(gamma), d(beta)
    z = (raw - mean) * rstd * gamma + beta
    mag = (raw.abs() + mean.abs()) * rstd.abs() * gamma.abs() + beta.abs()
    return z, z.clamp_min(0.0), mag


def pyr_maxpool(x):
    return maxpool2_fwd(_even(d(x)).unsqueeze(-1)).squeeze(-1)


def _even(x):
    """Floor mode: the last row / column of an odd map is in no window."""
    return x[:, :x.shape[1] // 2 * 2, :x.shape[2] // 2 * 2]


def bil_coord(n_in, n_out):
    """pyr_bil_coord for every output index: i0, i1 (int64) and l (float32, as the kernel forms it)."""
    o = torch.arange(n_out, dtype=torch.float32)
    sc = (torch.tensor(float(n_in - 1), dtype=torch.float32) / torch.tensor(float(n_out - 1), dtype=torch.float32)) if n_out > 1 else torch.tensor(0.0)
    f = sc.to(torch.float32) * o
    i0 = f.to(torch.int64).clamp_max(n_in - 1)
    i1 = i0 + (i0 < n_in - 1).to(torch.int64)
    l = f - i0.to(torch.float32)
    return i0, i1, l


RESIZE_K = 11 + 2       # 1 - ly, 1 - lx, four inner products, two inner sums, two outer products, one sum


def pyr_resize(x, OH, OW):
    """align_corners=True bilinear resize of [N, IH, IW] -> ref, mag."""
    x = d(x)
    y0, y1, ly = bil_coord(x.shape[1], OH)
    x0, x1, lx = bil_coord(x.shape[2], OW)
    ly, lx = ly.to(_rd()).view(1, OH, 1), lx.to(_rd()).view(1, 1, OW)

    def blend(v):
        top = (1 - lx) * v[:, y0][:, :, x0] + lx * v[:, y0][:, :, x1]
        bot = (1 - lx) * v[:, y1][:, :, x0] + lx * v[:, y1][:, :, x1]
        return (1 - ly) * top + ly * bot
    return blend(x), blend(x.abs())


# ------------------------------------------------------------------------------------------------ the whole pyramid / FPA block in torch (autograd)
def pyramid_torch(x1raw, prm, train=True, dtype=torch.float64):
    """smp's FPABlock below its wide conv, restated from oracle/nets.py on NCHW maps: x1raw [N, h1, w1] (down1's conv output), the block's map
    h x w.  prm: w, b, gamma, beta (lists of 6; w[0] / b[0] unused), optionally rm, rv for eval.  -> uu [N, h, w], dict of intermediates."""
    up = dict(mode='bilinear', align_corners=True)
    h, w = prm['hw']
    it = {}

    def cbr(x, l, name, conv=True):
        if conv:
            x = F.conv2d(x, prm['w'][l].to(dtype).view(1, 1, PYR_K[l], PYR_K[l]), prm['b'][l].to(dtype).view(1), padding=PYR_K[l] // 2)
        if train:
            z = F.batch_norm(x, None, None, prm['gamma'][l].to(dtype).view(1), prm['beta'][l].to(dtype).view(1), True, 0.0, BN_EPS)
        else:
            z = F.batch_norm(x, prm['rm'][l].to(dtype).view(1), prm['rv'][l].to(dtype).view(1), prm['gamma'][l].to(dtype).view(1),
                             prm['beta'][l].to(dtype).view(1), False, 0.0, BN_EPS)
        it['raw_' + name], it['z_' + name] = x, z
        return F.relu(z)
    x1 = cbr(x1raw.to(dtype).unsqueeze(1), 0, 'down1', conv=False)
    x2 = cbr(F.max_pool2d(x1, 2, 2), 1, 'down2')
    x3 = cbr(cbr(F.max_pool2d(x2, 2, 2), 2, 'down3a'), 3, 'down3b')
    it['x1'], it['x2'] = x1, x2
    x3u = F.interpolate(x3, size=(h // 4, w // 4), **up)
    t = cbr(x2, 4, 'conv2') + x3u
    u = F.interpolate(t, size=(h // 2, w // 2), **up) + cbr(x1, 5, 'conv1')
    uu = F.interpolate(u, size=(h, w), **up)
    it.update(x3=x3, x3u=x3u, t=t, u=u)
    return uu.squeeze(1), it


def kink_margins(it):
    """Smallest |z| in front of the six ReLUs, and the smallest lead of a POSITIVE max-pool winner over its runner-up (windows tied at 0
    after the ReLU pass no gradient: harmless)."""
    zmin = min(float(v.detach().abs().min()) for k, v in it.items() if k.startswith('z_'))
    lead = float('inf')
    for k in ('x1', 'x2'):
        x = it[k].detach()[:, 0]
        q = _quads(_even(x).unsqueeze(-1)).squeeze(-1)
        top2 = q.topk(2, dim=0).values
        pos = top2[0] > 0
        if bool(pos.any()):
            lead = min(lead, float((top2[0] - top2[1])[pos].min()))
    return zmin, lead


def unit_off_fractions(it):
    return {k: float((v.detach() <= 0).double().mean()) for k, v in it.items() if k.startswith('z_')}


def pyramid_grads(x1raw, prm, duu, dtype=torch.float64, start=None):
    """Autograd of sum(uu duu): -> dict dx1raw, dw{l}, db{l} (l = 1..5), dgamma{l}, dbeta{l} (l = 0..5), each + its starting value."""
    leaf = lambda t: t.detach().clone().to(dtype).requires_grad_(True)      # noqa: E731
    x = leaf(x1raw)
    p = dict(hw=prm['hw'], w=[None] + [leaf(t) for t in prm['w'][1:]], b=[None] + [leaf(t) for t in prm['b'][1:]],
             gamma=[leaf(t) for t in prm['gamma']], beta=[leaf(t) for t in prm['beta']])
    uu, it = pyramid_torch(x, p, True, dtype)
    (uu * duu.to(dtype)).sum().backward()
    out = dict(dx1raw=x.grad)
    for l in range(6):
        if l >= 1:
            out[f'dw{l}'], out[f'db{l}'] = p['w'][l].grad, p['b'][l].grad
        out[f'dgamma{l}'], out[f'dbeta{l}'] = p['gamma'][l].grad, p['beta'][l].grad
    if start is not None:
        for k in out:
            if k in start:
                out[k] = (out[k].reshape(-1) + start[k].to(dtype).reshape(-1))
    return out, it


def fpa_block_grads(x, w0, b0, prm, mid, b1, g, dtype=torch.float64, T=torch.float32, start=None):
    """The FPA block from its input feature on: maxpool2 -> wide 7x7 conv -> pyramid -> uu * mid + b1; autograd of sum(out g).
    x [N, H, W, C], mid [N, HW, Cm], b1 [N, Cm], g [N, HW, Cm] (NHWC); dtype: the arithmetic, T: where the kernels store T the float32
    yardstick stores T too (p, out; the float64 reference rounds nothing)."""
    leaf = lambda t: t.detach().clone().to(dtype).requires_grad_(True)      # noqa: E731
    xs, w0s, b0s, mids, b1s = leaf(x), leaf(w0), leaf(b0), leaf(mid), leaf(b1)
    N, H, W, Cn = x.shape
    p = dict(hw=(H, W), w=[None] + [leaf(t) for t in prm['w'][1:]], b=[None] + [leaf(t) for t in prm['b'][1:]],
             gamma=[leaf(t) for t in prm['gamma']], beta=[leaf(t) for t in prm['beta']])
    pooled = F.max_pool2d(xs.permute(0, 3, 1, 2), 2, 2)
    x1raw = F.conv2d(pooled, w0s.view(7, 7, Cn).permute(2, 0, 1).unsqueeze(0).contiguous(), b0s.view(1), padding=3)[:, 0]
    uu, it = pyramid_torch(x1raw, p, True, dtype)
    out = uu.reshape(N, H * W, 1) * mids + b1s.unsqueeze(1)
    (out * g.to(dtype)).sum().backward()
    res = dict(dx=xs.grad, dw0=w0s.grad.reshape(-1), db0=b0s.grad, dmid=mids.grad, dbranch1=b1s.grad)
    for l in range(6):
        if l >= 1:
            res[f'dw{l}'], res[f'db{l}'] = p['w'][l].grad, p['b'][l].grad
        res[f'dgamma{l}'], res[f'dbeta{l}'] = p['gamma'][l].grad, p['beta'][l].grad
    if start is not None:
        for k in res:
            if k in start:
                res[k] = res[k].reshape(-1) + start[k].to(dtype).reshape(-1)
    if dtype == torch.float32 and T != torch.float32:
        for k in ('dx', 'dmid', 'dbranch1'):
            res[k] = res[k].to(T).to(dtype)
    return res, it, out.detach()


def yardstick_check(got, ref64, yard32, what, dtype_name='f32'):
    """The pyramid backward's rule: per tensor, max |got - ref64| <= max(4 x max |yard32 - ref64|, 16 eps32 max |ref64|)."""
    g = got.detach().cpu().to(torch.float64).reshape(-1)
    r = ref64.detach().to(torch.float64).reshape(-1)
    y = yard32.detach().to(torch.float64).reshape(-1)
    assert bool(torch.isfinite(g).all()), f'{what}: non-finite elements'
    kd, yd = float((g - r).abs().max()), float((y - r).abs().max())
    floor = 16 * R.EPS32 * float(r.abs().max())
    bound = max(4 * yd, floor)
    R.RATIOS.append((what, dtype_name, kd / bound if bound > 0 else (0.0 if kd == 0 else float('inf'))))
    print(f'yardstick {what} {dtype_name}: kernel {kd:.3e}, float32 yardstick {yd:.3e}, floor {floor:.3e}')
    assert kd <= bound, f'{what}: kernel {kd:.3e} from float64, yardstick {yd:.3e}, floor {floor:.3e}'


# ------------------------------------------------------------------------------------------------ fpa_mix
MIX_K = 2 + 2


def fpa_mix_fwd(uu, mid, b1):
    uu, mid, b1 = d(uu), d(mid), d(b1)
    prod = uu.unsqueeze(-1) * mid
    return prod + b1.unsqueeze(1), prod.abs() + b1.abs().unsqueeze(1)


def fpa_mix_bwd(uu, mid, g):
    """-> (dmid, mag), (duu, sum|terms|); duu: C terms."""
    uu, mid, g = d(uu), d(mid), d(g)
    dmid = g * uu.unsqueeze(-1)
    return (dmid, dmid.abs()), ((g * mid).sum(-1), (g * mid).abs().sum(-1))


# ------------------------------------------------------------------------------------------------ pab_gemm (flat strided operands)
def _operand(flat, batch, sb, rows, sr, cols, sc):
    idx = (torch.arange(batch).view(-1, 1, 1) * sb + torch.arange(rows).view(1, -1, 1) * sr + torch.arange(cols).view(1, 1, -1) * sc)
    return d(flat).reshape(-1)[idx], idx


def pab_gemm(g, batch, A, B, C0=None):
    """g: blockops.Gemm.  -> ref (the whole flat C buffer, untouched elements = C0 or NaN), sum|terms|, written (bool mask)."""
    a, _ = _operand(A, batch, g.sA[0], g.M, g.sA[1], g.K, g.sA[2])
    b, _ = _operand(B, batch, g.sB[0], g.K, g.sB[1], g.N, g.sB[2])
    prod = torch.einsum('bmk,bkn->bmn', a, b)
    sa = torch.einsum('bmk,bkn->bmn', a.abs(), b.abs())
    _, cidx = _operand(torch.zeros(batch * g.numelC), batch, g.sC[0], g.M, g.sC[1], g.N, g.sC[2])
    if C0 is not None:
        c0 = d(C0).reshape(-1)[cidx]
        prod, sa = prod + c0, sa + c0.abs()
    ref = torch.full((batch * g.numelC,), float('nan'), dtype=_rd())
    sab = torch.zeros(batch * g.numelC, dtype=_rd())
    ref[cidx.reshape(-1)] = prod.reshape(-1)
    sab[cidx.reshape(-1)] = sa.reshape(-1)
    return ref, sab


# ------------------------------------------------------------------------------------------------ pab_softmax
SOFTMAX_K = 4 + 2       # s - max, exp, the sum's reciprocal, the product
SOFTMAX_BWD_K = 3 + 2   # the dot's rounding to float, dP - dot, P * .


def pab_softmax_fwd(S):
    s = d(S)
    e = torch.exp(s - s.max(1, keepdim=True).values)
    return e / e.sum(1, keepdim=True)


def pab_softmax_bwd(dP, P):
    dP, P = d(dP), d(P)
    dot = (P * dP).sum(1, keepdim=True)
    return P * (dP - dot), P * (dP.abs() + (P * dP).abs().sum(1, keepdim=True))


# ------------------------------------------------------------------------------------------------ pab_mix
def pab_mix_index(N, HW, Cn):
    """flat index into M [N, HW * C] that y[n, p, ch] reads: ch * HW + p (the un-transposed reshape)."""
    return (torch.arange(Cn).view(1, 1, Cn) * HW + torch.arange(HW).view(1, HW, 1)).expand(N, HW, Cn)


def pab_mix_fwd(x, M):
    x, M = d(x), d(M)
    N, HW, Cn = x.shape
    m = torch.gather(M.reshape(N, HW * Cn), 1, pab_mix_index(N, HW, Cn).reshape(N, -1)).view(N, HW, Cn)
    return x + m, x.abs() + m.abs()


def pab_mix_bwd(dy):
    dy = d(dy)
    N, HW, Cn = dy.shape
    out = torch.zeros(N, HW * Cn, dtype=dy.dtype)
    out.scatter_(1, pab_mix_index(N, HW, Cn).reshape(N, -1), dy.reshape(N, -1))
    return out


def pab_torch(x, center, top, bottom, dtype=torch.float64):
    """smp's PAB between its convs, restated from oracle/nets.py: x, bottom [N, HW, C], center, top [N, HW, 64] (NHWC = the transposed
    flattened NCHW maps) -> y [N, HW, C] (NHWC), and S, P, M."""
    N, HW, Cn = x.shape
    S = torch.matmul(center.to(dtype), top.to(dtype).transpose(1, 2))
    P = torch.softmax(S.view(N, -1), dim=1).view(N, HW, HW)
    M = torch.matmul(P, bottom.to(dtype))
    y = x.to(dtype).transpose(1, 2) + M.reshape(N, Cn, HW)      # NCHW with the map flattened
    return y.transpose(1, 2), S, P, M
