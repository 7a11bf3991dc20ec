"""The case table of the single-stage tests of pan.hip's pyramid kernels and pab.hip's attention kernels.

One family per launcher (or chain); FAMILIES[name]() -> list of Case.  A Case holds its CPU inputs (`ins`), its device outputs (`outs`:
name -> (shape, dtype, init); init None = starts as NaN), the call(s) on blockops (`call(B, t)`, t: name -> guarded device tensor) and
either `refs()` (Rule X: name -> float64 reference, compared bit for bit after ONE rounding) or `check(t)` (t: name -> CPU tensor after
the call; Rules E / R / T of sweep_ref.py, every one appending to sweep_ref.RATIOS).  No map is larger than 22 x 22 and no C larger
than 264.  tests/test_blockops.py proves the Rule X input sets exact in float32 and the kink margins of the pyramid seeds;
tests/test_gpu_blockops.py runs the table on the GPU.
"""
import torch

import block_ref as BR
import sweep_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import blockops as B_
from sweep_cases import Case, _seed

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
TRAIN_DTYPES = (F32, BF16)
FWD_DTYPES = (F32, BF16, F16)
NAME = R.DTYPE_NAMES
CODE = {F32: L.F32, BF16: L.BF16, F16: L.F16}
PYR_K = BR.PYR_K


def _ratio(what, dtype, got, ref, bound):
    """Rule E / R comparison that also records the worst error / bound ratio."""
    g = R.d(got).reshape(ref.shape)
    err = (g - ref).abs()
    ok = bound > 0
    r = float((err[ok] / bound[ok]).max()) if bool(ok.any()) else 0.0
    R.RATIOS.append((what, NAME[dtype], r if r == r else float('inf')))
    R.assert_within(got, ref, bound, what)


def _finite(t, names):
    for k in names:
        assert bool(torch.isfinite(t[k].float()).all()), f'{k}: an owned element is not finite'


def _bits_equal(a, b, what):
    assert torch.equal(R.bits_of(a.cpu()), R.bits_of(b.cpu())), f'{what}: not bit-identical'


# =============================================================================================== maxpool2
MAXPOOL_SHAPES = ((2, 4, 6, 8), (1, 2, 2, 16), (3, 6, 4, 24))


def _maxpool_x(shape, T, g):
    x = R.dyadic(shape, T, g, -8, 8, 0.5)      # 17 values over 4 window places: ties abound
    x[0, 0:2, 0:2, :] = float('-inf')          # a window of -inf in every channel
    x[-1, -2:, -2:, ::3] = float('-inf')
    x[-1, -1, -1, 1] = float('-inf')           # and a lone -inf that must lose
    return x


def maxpool2_cases():
    cases = []
    for shape in MAXPOOL_SHAPES:
        N, H, W, Cn = shape
        ps = (N, H // 2, W // 2, Cn)
        for T in FWD_DTYPES:
            g = R.gen(_seed('maxpool2', shape, NAME[T]))
            x = _maxpool_x(shape, T, g)
            cases.append(Case(f'maxpool2_fwd-{N}x{H}x{W}x{Cn}-{NAME[T]}', T, dict(x=x), dict(p=(ps, T, None)),
                              lambda B, t: B.maxpool2_fwd(t['x'], t['p']), refs=lambda x=x: dict(p=BR.maxpool2_fwd(x))))
            if T == F16:
                continue
            dp = R.dyadic(ps, T, g)
            dx0 = R.dyadic(shape, T, g)
            cases.append(Case(f'maxpool2_bwd-store-{N}x{H}x{W}x{Cn}-{NAME[T]}', T, dict(x=x, dp=dp), dict(dx=(shape, T, None)),
                              lambda B, t: B.maxpool2_bwd(t['x'], t['dp'], t['dx'], 0), refs=lambda x=x, dp=dp: dict(dx=BR.maxpool2_bwd(x, dp))))
            cases.append(Case(f'maxpool2_bwd-accum-{N}x{H}x{W}x{Cn}-{NAME[T]}', T, dict(x=x, dp=dp), dict(dx=(shape, T, dx0)),
                              lambda B, t: B.maxpool2_bwd(t['x'], t['dp'], t['dx'], 1),
                              refs=lambda x=x, dp=dp, dx0=dx0: dict(dx=BR.maxpool2_bwd(x, dp, dx0))))
    return cases


# =============================================================================================== fpa_in_fwd / fpa_in_bwd
IN_SHAPES = ((2, 4, 4, 8), (1, 2, 3, 264), (2, 11, 7, 40))
IN_K = 7


def fpa_in_cases():
    cases = []
    K = IN_K
    for shape in IN_SHAPES:
        N, H, W, Cn = shape
        sid = f'{N}x{H}x{W}x{Cn}'
        for T in FWD_DTYPES:
            g = R.gen(_seed('fpa_in', shape, NAME[T]))
            # ---- Rule X twin: dyadic p (quarters up to 2), integer w: every sum below 49 C 8 < 2^24 quarter units
            p = R.dyadic(shape, T, g)
            w = R.ints((K * K, Cn), g)
            b = R.ints((1,), g)
            cases.append(Case(f'fpa_in_fwd-exact-{sid}-{NAME[T]}', T, dict(p=p, w=w, b=b), dict(y=((N, H, W), F32, None)),
                              lambda B, t: B.fpa_in_fwd(t['p'], t['w'], t['b'], t['y'], IN_K),
                              refs=lambda p=p, w=w, b=b: dict(y=BR.fpa_in_fwd(p, w, b, IN_K)[0])))
            # ---- Rule R: Gaussian operands, n = 49 C + 1 terms
            pg, wg, bg = R.normal(shape, T, g), R.normal((K * K, Cn), F32, g, 0.1), R.normal((1,), F32, g)

            def check_fwd(t, pg=pg, wg=wg, bg=bg, T=T, Cn=Cn):
                ref, sa = BR.fpa_in_fwd(pg, wg, bg, IN_K)
                _ratio('fpa_in_fwd y', T, t['y'], ref, R.bound_r(ref, sa, IN_K * IN_K * Cn + 1))
            cases.append(Case(f'fpa_in_fwd-{sid}-{NAME[T]}', T, dict(p=pg, w=wg, b=bg), dict(y=((N, H, W), F32, None)),
                              lambda B, t: B.fpa_in_fwd(t['p'], t['w'], t['b'], t['y'], IN_K), check=check_fwd))
            if T == F16:
                continue
            dy = R.ints((N, H, W), g)
            dw0, db0 = R.ints((K * K, Cn), g), R.ints((1,), g, 1, 4)
            outs = dict(dp=(shape, T, None), dw=((K * K, Cn), F32, dw0), db=((1,), F32, db0))
            call = lambda B, t: B.fpa_in_bwd(t['p'], t['dy'], t['w'], t['dp'], t['dw'], t['db'], IN_K)      # noqa: E731

            def refs_bwd(p=p, dy=dy, w=w, dw0=dw0, db0=db0):
                r = BR.fpa_in_bwd(p, dy, w, dw0, db0, IN_K)
                return {k: v[0] for k, v in r.items()}
            cases.append(Case(f'fpa_in_bwd-exact-{sid}-{NAME[T]}', T, dict(p=p, dy=dy, w=w), outs, call, refs=refs_bwd))
            dyg = R.normal((N, H, W), F32, g)
            dw0g, db0g = R.normal((K * K, Cn), F32, g) + 2.0, R.normal((1,), F32, g) + 3.0
            outs_g = dict(dp=(shape, T, None), dw=((K * K, Cn), F32, dw0g), db=((1,), F32, db0g))

            def check_bwd(t, pg=pg, dyg=dyg, wg=wg, dw0g=dw0g, db0g=db0g, T=T, n=N * H * W):
                r = BR.fpa_in_bwd(pg, dyg, wg, dw0g, db0g, IN_K)
                _ratio('fpa_in_bwd dp', T, t['dp'], r['dp'][0], R.bound_r(r['dp'][0], r['dp'][1], IN_K * IN_K, T))
                _ratio('fpa_in_bwd dw', T, t['dw'], r['dw'][0], R.bound_r(r['dw'][0], r['dw'][1], n + 1))
                _ratio('fpa_in_bwd db', T, t['db'], r['db'][0], R.bound_r(r['db'][0], r['db'][1], n + 1))
            cases.append(Case(f'fpa_in_bwd-{sid}-{NAME[T]}', T, dict(p=pg, dy=dyg, w=wg), outs_g, call, check=check_bwd))
    return cases


# =============================================================================================== the pyramid
PYR_SHAPES = ((2, 8, 8), (3, 22, 14), (2, 16, 24))
PYR_SEED = {(2, 8, 8): 1, (3, 22, 14): 1, (2, 16, 24): 2}      # test_blockops.py asserts their kink margins
KINK = 1e-3


def pyr_inputs(N, h, w, seed):
    """The issue's recipe: unit-Gaussian x1raw, conv weights 1.5 / k N(0, 1), gamma 1 +- 0.3, beta 0.2 +- 0.3 (all float32)."""
    g = R.gen(seed)
    (_, (h1, w1), _, _), _ = B_.fpa_levels(N, h, w)
    x1raw = R.normal((N, h1, w1), F32, g)
    prm = dict(hw=(h, w), w=[None], b=[None])
    for l in range(1, 6):
        prm['w'].append(R.normal((PYR_K[l] ** 2,), F32, g, 1.5 / PYR_K[l]))
        prm['b'].append(R.normal((1,), F32, g, 0.1))
    prm['gamma'] = list((1.0 + 0.3 * R.normal((6,), F32, g).clamp(-1, 1)).split(1))
    prm['beta'] = list((0.2 + 0.3 * R.normal((6,), F32, g).clamp(-1, 1)).split(1))
    prm['rm'] = list((0.25 * R.normal((6,), F32, g)).split(1))
    prm['rv'] = list((1.0 + 0.5 * torch.rand(6, generator=g, dtype=torch.float64).to(F32)).split(1))
    duu = R.normal((N, h, w), F32, g)
    return x1raw, prm, duu


def _pyr_ins(prm):
    ins = {f'w{l}': prm['w'][l] for l in range(1, 6)}
    ins.update(b=torch.cat([torch.zeros(1)] + prm['b'][1:]), gamma=torch.cat(prm['gamma']), beta=torch.cat(prm['beta']))
    return ins


def _pyr_scratch0(N, h, w, x1raw):
    s = torch.full((B_.fpa_scratch_floats(N, h, w),), float('nan'))
    s[:x1raw.numel()] = x1raw.reshape(-1)
    return s


def _dev_prm(t, sfx=''):
    sp = lambda k: [t[k][l:l + 1] for l in range(6)]      # noqa: E731
    return dict(w=[None] + [t[f'w{l}'] for l in range(1, 6)], b=[None] + sp('b')[1:], gamma=sp('gamma'), beta=sp('beta'), rm=sp('rm' + sfx), rv=sp('rv' + sfx))


def _check_pyr_fwd(t, N, h, w, prm, train, tag):
    dims, ns = B_.fpa_levels(N, h, w)
    v = B_.fpa_scratch_views(N, h, w, t['scratch'])
    names = [k for k in v if k not in ('stats', 'spare')]
    _finite(v, names)
    assert bool(torch.isnan(v['spare']).all()), 'the spare floats behind the statistics were written'
    _bits_equal(t['scratch'], t['scratch2'], f'{tag}: the second launch')
    _bits_equal(t['rm'], t['rm2'], f'{tag}: running mean of the second launch')
    _bits_equal(t['rv'], t['rv2'], f'{tag}: running var of the second launch')
    T = F32
    gam, bet = prm['gamma'], prm['beta']

    def conv(src, dst, l):
        ref, sa = BR.pyr_conv(v[src], prm['w'][l], prm['b'][l], PYR_K[l])
        _ratio(f'pyr_conv{PYR_K[l]} {tag}', T, v[dst], ref, R.bound_r(ref, sa, PYR_K[l] ** 2 + 1))

    def bn(raw, out, l):
        x = v[raw]
        n = x.numel()
        mean, var, unb, amean = BR.pyr_bn_stats(x)
        if train:
            km, kr = v['stats'][2 * l], v['stats'][2 * l + 1]
            _ratio(f'pyr_bn mean {tag}', T, km, mean, R.bound_r(mean, amean, n + 1, F32))
            rstd = 1.0 / torch.sqrt(var + BR.BN_EPS)
            yard = (1.0 / torch.sqrt(var.to(F32) + BR.BN_EPS)).to(F32)
            R.assert_transcendental(kr, rstd, yard, R.bound_e(rstd, rstd, 3 + 2, F32), f'pyr_bn rstd {tag}', F32)
            # the running statistics, from known non-trivial starting values; the unbiased variance goes into running_var
            rm0, rv0 = R.d(prm['rm'][l])[0], R.d(prm['rv'][l])[0]
            ref_rm, ref_rv = (1 - BR.BN_MOM) * rm0 + BR.BN_MOM * mean, (1 - BR.BN_MOM) * rv0 + BR.BN_MOM * unb
            _ratio(f'pyr_bn running_mean {tag}', T, t['rm'][l], ref_rm, R.bound_e(ref_rm, 0.9 * rm0.abs() + 0.1 * mean.abs(), BR.RUN_K, F32))
            _ratio(f'pyr_bn running_var {tag}', T, t['rv'][l], ref_rv, R.bound_e(ref_rv, 0.9 * rv0.abs() + 0.1 * unb, BR.RUN_K, F32))
            k = BR.BN_OUT_K
        else:
            km = prm['rm'][l][0]
            kr = 1.0 / torch.sqrt(R.d(prm['rv'][l])[0] + BR.BN_EPS)
            k = BR.BN_EVAL_K
        z, ref, mag = BR.pyr_bn_relu_out(x, km, kr, gam[l][0], bet[l][0])
        # (where |z| lies below its bound the kernel's own sign decides between 0 and z: both lie within the bound of relu(z))
        _ratio(f'pyr_bn_relu {tag}', T, v[out], ref, R.bound_e(ref, mag, k, F32))

    def pool(src, dst):
        R.assert_exact(v[dst], BR.pyr_maxpool(v[src]), f'{tag} maxpool {dst}')

    def resize(src, dst, lvl, add=None):
        ref, mag = BR.pyr_resize(v[src], *dims[lvl])
        k = BR.RESIZE_K
        if add is not None:
            ref, mag, k = ref + R.d(v[add]), mag + R.d(v[add]).abs(), k + 1
        _ratio(f'pyr_resize {tag}', T, v[dst], ref, R.bound_e(ref, mag, k, F32))

    bn('r1', 'x1', 0)
    pool('x1', 'p2')
    conv('p2', 'r2', 1)
    bn('r2', 'x2', 1)
    pool('x2', 'p3')
    conv('p3', 'r3a', 2)
    bn('r3a', 'x3a', 2)
    conv('x3a', 'r3b', 3)
    bn('r3b', 'x3', 3)
    resize('x3', 'x3u', 2)
    conv('x2', 'c2', 4)
    bn('c2', 'y2', 4)
    ref = R.d(v['y2']) + R.d(v['x3u'])
    _ratio(f'pyr_add {tag}', T, v['t'], ref, R.bound_e(ref, R.d(v['y2']).abs() + R.d(v['x3u']).abs(), 1 + 2, F32))
    conv('x1', 'c1', 5)
    bn('c1', 'y1', 5)
    resize('t', 'tu', 1, add='y1')           # tu holds u = up(t) + y1 when the kernel ends
    resize('tu', 'uu', 0)
    if train:
        _finite(v, ['stats'])
    else:
        assert bool(torch.isnan(v['stats']).all()), 'eval wrote the statistics'
        _bits_equal(t['rm'], torch.cat(prm['rm']), 'eval: running mean')
        _bits_equal(t['rv'], torch.cat(prm['rv']), 'eval: running var')


def fpa_pyr_fwd_cases():
    cases = []
    for (N, h, w) in PYR_SHAPES:
        x1raw, prm, _ = pyr_inputs(N, h, w, PYR_SEED[(N, h, w)])
        for train in (1, 0):
            for T in TRAIN_DTYPES:      # the pyramid is float32 whatever the dtype: the door must take both
                s0 = _pyr_scratch0(N, h, w, x1raw)
                outs = dict(scratch=(s0.shape, F32, s0), scratch2=(s0.shape, F32, s0.clone()))
                for k in ('rm', 'rv'):
                    outs[k] = ((6,), F32, torch.cat(prm[k]))
                    outs[k + '2'] = ((6,), F32, torch.cat(prm[k]))

                def call(B, t, N=N, h=h, w=w, train=train, T=T):
                    B.fpa_pyr_fwd(t['scratch'], _dev_prm(t), N, h, w, train, CODE[T])
                    B.fpa_pyr_fwd(t['scratch2'], _dev_prm(t, '2'), N, h, w, train, CODE[T])
                tag = 'train' if train else 'eval'
                cases.append(Case(f'fpa_pyr_fwd-{tag}-{N}x{h}x{w}-{NAME[T]}', T, _pyr_ins(prm), outs, call,
                                  check=lambda t, N=N, h=h, w=w, prm=prm, train=train, tag=tag: _check_pyr_fwd(t, N, h, w, prm, train, tag)))
    return cases


GRAD_NAMES = [f'dw{l}' for l in range(1, 6)] + ['db', 'dgamma', 'dbeta']


def _grad_starts(g):
    st = {f'dw{l}': R.normal((PYR_K[l] ** 2,), F32, g) + 2.0 for l in range(1, 6)}
    st.update(db=R.normal((6,), F32, g) - 2.0, dgamma=R.normal((6,), F32, g) + 1.5, dbeta=R.normal((6,), F32, g) - 1.5)
    return st


def _start_per_layer(st):
    out = {f'dw{l}': st[f'dw{l}'] for l in range(1, 6)}
    for l in range(6):
        if l >= 1:
            out[f'db{l}'] = st['db'][l:l + 1]
        out[f'dgamma{l}'], out[f'dbeta{l}'] = st['dgamma'][l:l + 1], st['dbeta'][l:l + 1]
    return out


def _dev_grads(t, sfx=''):
    sp = lambda k: [t[k + sfx][l:l + 1] for l in range(6)]      # noqa: E731
    return dict(dw=[None] + [t[f'dw{l}' + sfx] for l in range(1, 6)], db=[None] + sp('db')[1:], dgamma=sp('dgamma'), dbeta=sp('dbeta'))


def _got_per_layer(t, sfx=''):
    out = {f'dw{l}': t[f'dw{l}' + sfx] for l in range(1, 6)}
    for l in range(6):
        if l >= 1:
            out[f'db{l}'] = t['db' + sfx][l:l + 1]
        out[f'dgamma{l}'], out[f'dbeta{l}'] = t['dgamma' + sfx][l:l + 1], t['dbeta' + sfx][l:l + 1]
    return out


def fpa_pyr_bwd_cases():
    cases = []
    for (N, h, w) in PYR_SHAPES:
        x1raw, prm, duu = pyr_inputs(N, h, w, PYR_SEED[(N, h, w)])
        st = _grad_starts(R.gen(_seed('pyr_bwd', N, h, w)))
        for T in TRAIN_DTYPES:
            s0 = _pyr_scratch0(N, h, w, x1raw)
            ng = B_.fpa_gscratch_floats(N, h, w)
            outs = {}
            for sfx in ('', '2'):
                outs['scratch' + sfx] = (s0.shape, F32, s0.clone())
                outs['gscratch' + sfx] = ((ng,), F32, None)
                for k in ('rm', 'rv'):
                    outs[k + sfx] = ((6,), F32, torch.cat(prm[k]))
                for k in GRAD_NAMES:
                    outs[k + sfx] = (st[k].shape, F32, st[k].clone())
            ins = _pyr_ins(prm)
            ins['duu'] = duu

            def call(B, t, N=N, h=h, w=w, T=T):
                for sfx in ('', '2'):
                    p = _dev_prm(t, sfx)
                    B.fpa_pyr_fwd(t['scratch' + sfx], p, N, h, w, 1, CODE[T])
                    p.update(_dev_grads(t, sfx))
                    B.fpa_pyr_bwd(t['scratch' + sfx], t['gscratch' + sfx], t['duu'], p, N, h, w, CODE[T])

            def check(t, N=N, h=h, w=w, T=T, x1raw=x1raw, prm=prm, duu=duu, st=st):
                _finite(t, ['gscratch'] + GRAD_NAMES)
                for k in ['scratch', 'gscratch'] + GRAD_NAMES:
                    _bits_equal(t[k], t[k + '2'], f'{k}: the second launch')
                assert float(t['db'][0]) == float(st['db'][0]), 'db of layer 0 belongs to fpa_in_bwd'
                start = _start_per_layer(st)
                ref, _ = BR.pyramid_grads(x1raw, prm, duu, torch.float64, start)
                yard, _ = BR.pyramid_grads(x1raw, prm, duu, torch.float32, start)
                got = _got_per_layer(t)
                got['dx1raw'] = B_.fpa_gscratch_views(N, h, w, t['gscratch'])['dx1']
                for k in sorted(ref):
                    BR.yardstick_check(got[k], ref[k], yard[k], f'pyr_bwd-{k} {N}x{h}x{w}', NAME[T])
            cases.append(Case(f'fpa_pyr_bwd-{N}x{h}x{w}-{NAME[T]}', T, ins, outs, call, check=check))
    return cases


# =============================================================================================== fpa_mix
MIX_SHAPES = ((2, 12, 32), (1, 5, 8), (3, 64, 32))


def fpa_mix_cases():
    cases = []
    for shape in MIX_SHAPES:
        N, HW, Cn = shape
        sid = f'{N}x{HW}x{Cn}'
        for T in FWD_DTYPES:
            g = R.gen(_seed('fpa_mix', shape, NAME[T]))
            uu, mid, b1 = R.dyadic((N, HW), F32, g), R.dyadic(shape, T, g), R.dyadic((N, Cn), T, g)
            fwd = lambda B, t: B.fpa_mix_fwd(t['uu'], t['mid'], t['b1'], t['out'])      # noqa: E731
            cases.append(Case(f'fpa_mix_fwd-exact-{sid}-{NAME[T]}', T, dict(uu=uu, mid=mid, b1=b1), dict(out=(shape, T, None)), fwd,
                              refs=lambda uu=uu, mid=mid, b1=b1: dict(out=BR.fpa_mix_fwd(uu, mid, b1)[0])))
            uug, midg, b1g = R.normal((N, HW), F32, g), R.normal(shape, T, g), R.normal((N, Cn), T, g)

            def check_fwd(t, uug=uug, midg=midg, b1g=b1g, T=T):
                ref, mag = BR.fpa_mix_fwd(uug, midg, b1g)
                _ratio('fpa_mix_fwd out', T, t['out'], ref, R.bound_e(ref, mag, BR.MIX_K, T))
            cases.append(Case(f'fpa_mix_fwd-{sid}-{NAME[T]}', T, dict(uu=uug, mid=midg, b1=b1g), dict(out=(shape, T, None)), fwd, check=check_fwd))
            if T == F16:
                continue
            gg = R.normal(shape, T, g)
            gx = R.dyadic(shape, T, g)
            bwd = lambda B, t: B.fpa_mix_bwd(t['uu'], t['mid'], t['g'], t['dmid'], t['duu'])      # noqa: E731
            outs = dict(dmid=(shape, T, None), duu=((N, HW), F32, None))

            def refs_bwd(uu=uu, mid=mid, gx=gx):
                (dm, _), (du, _) = BR.fpa_mix_bwd(uu, mid, gx)
                return dict(dmid=dm, duu=du)
            cases.append(Case(f'fpa_mix_bwd-exact-{sid}-{NAME[T]}', T, dict(uu=uu, mid=mid, g=gx), outs, bwd, refs=refs_bwd))

            def check_bwd(t, uug=uug, midg=midg, gg=gg, T=T, Cn=Cn):
                (dm, dmm), (du, dua) = BR.fpa_mix_bwd(uug, midg, gg)
                _ratio('fpa_mix_bwd dmid', T, t['dmid'], dm, R.bound_e(dm, dmm, 1 + 2, T))
                _ratio('fpa_mix_bwd duu', T, t['duu'], du, R.bound_r(du, dua, Cn))
            cases.append(Case(f'fpa_mix_bwd-{sid}-{NAME[T]}', T, dict(uu=uug, mid=midg, g=gg), outs, bwd, check=check_bwd))
    return cases


# =============================================================================================== the FPA chain (the plan's order and offsets)
CHAIN = (2, 8, 8, 16)
CHAIN_MID = 16
CHAIN_SEED = 1


def chain_inputs(T):
    N, H, W, Cn = CHAIN
    _, prm, _ = pyr_inputs(N, H, W, CHAIN_SEED)
    g = R.gen(_seed('fpa_chain', CHAIN_SEED))
    x = R.normal(CHAIN, T, g)
    w0 = R.normal((49, Cn), F32, g, 1.0 / (7.0 * Cn ** 0.5) * 2.0)
    b0 = R.normal((1,), F32, g, 0.1)
    mid, b1 = R.normal((N, H * W, CHAIN_MID), T, g), R.normal((N, CHAIN_MID), T, g)
    gout = R.normal((N, H * W, CHAIN_MID), T, g)
    return x, w0, b0, prm, mid, b1, gout


def fpa_chain_cases():
    from oct_segmentation_amd import sweeps as S
    cases = []
    N, H, W, Cn = CHAIN
    n1 = N * (H // 2) * (W // 2)
    for T in TRAIN_DTYPES:
        x, w0, b0, prm, mid, b1, gout = chain_inputs(T)
        st = _grad_starts(R.gen(_seed('chain', NAME[T])))
        dw00, db00 = R.normal((49, Cn), F32, R.gen(5)) + 2.0, torch.tensor([1.25])
        ns, ng = B_.fpa_scratch_floats(N, H, W), B_.fpa_gscratch_floats(N, H, W)
        ins = _pyr_ins(prm)
        ins.update(x=x, w0=w0, b0=b0, mid=mid, b1=b1, gout=gout)
        outs = dict(p=((N, H // 2, W // 2, Cn), T, None), scratch=((ns,), F32, None), gs=((ng + N * H * W,), F32, None), out=((N, H * W, CHAIN_MID), T, None),
                    dmid=((N, H * W, CHAIN_MID), T, None), db1=((N, CHAIN_MID), T, None), dp=((N, H // 2, W // 2, Cn), T, None), dx=(CHAIN, T, None),
                    dw0=((49, Cn), F32, dw00), db0=((1,), F32, db00), rm=((6,), F32, torch.cat(prm['rm'])), rv=((6,), F32, torch.cat(prm['rv'])))
        for k in GRAD_NAMES:
            outs[k] = (st[k].shape, F32, st[k].clone())

        def call(B, t, T=T):
            uu_off = B.fpa_uu_offset(N, H, W)
            scr, gs = t['scratch'], t['gs']
            uu = scr[uu_off:uu_off + N * H * W]
            duu = gs[ng:]
            p = _dev_prm(t)
            # forward, as plan_forward.cpp OP_FPA
            B.maxpool2_fwd(t['x'], t['p'])
            B.fpa_in_fwd(t['p'], t['w0'], t['b0'], scr[:n1], 7)
            B.fpa_pyr_fwd(scr, p, N, H, W, 1, CODE[T])
            B.fpa_mix_fwd(uu, t['mid'], t['b1'], t['out'])
            # backward, as plan_backward.cpp OP_FPA
            B.fpa_mix_bwd(uu, t['mid'], t['gout'], t['dmid'], duu)
            S.image_sum(t['gout'], t['db1'], 1.0)
            p.update(_dev_grads(t))
            B.fpa_pyr_bwd(scr, gs[:ng], duu, p, N, H, W, CODE[T])
            B.fpa_in_bwd(t['p'], gs[n1:2 * n1], t['w0'], t['dp'], t['dw0'], t['db0'], 7)
            B.maxpool2_bwd(t['x'], t['dp'], t['dx'], 0)

        def check(t, T=T, x=x, w0=w0, b0=b0, prm=prm, mid=mid, b1=b1, gout=gout, st=st, dw00=dw00, db00=db00):
            _finite(t, ['p', 'gs', 'out', 'dmid', 'db1', 'dp', 'dx', 'dw0', 'db0'] + GRAD_NAMES)
            _finite(dict(scratch=t['scratch'][:-4]), ['scratch'])      # (the four spare floats behind the statistics belong to nobody)
            assert bool(torch.isnan(t['scratch'][-4:]).all())
            start = _start_per_layer(st)
            start.update(dw0=dw00, db0=db00)
            ref, _, out64 = BR.fpa_block_grads(x, w0, b0, prm, mid, b1, gout, torch.float64, T, start)
            yard, _, out32 = BR.fpa_block_grads(x, w0, b0, prm, mid, b1, gout, torch.float32, T, start)
            got = _got_per_layer(t)
            got.update(dx=t['dx'], dw0=t['dw0'], db0=t['db0'], dmid=t['dmid'], dbranch1=t['db1'])
            BR.yardstick_check(t['out'], out64, out32.to(T), 'fpa_chain-out', NAME[T])
            for k in sorted(ref):
                BR.yardstick_check(got[k], ref[k], yard[k], f'fpa_chain-{k}', NAME[T])
        cases.append(Case(f'fpa_chain-{NAME[T]}', T, ins, outs, call, check=check))
    return cases


# =============================================================================================== pab_gemm
GEMM_SHAPES = ((9, 8), (20, 24))
GEMM_BATCH = 2
FWD_SETS = ('S', 'M')


def _gemm_operands(gm, batch, T, g, exact):
    mk = (lambda n, dt: R.dyadic((n,), dt, g)) if exact else (lambda n, dt: R.normal((n,), dt, g))
    A = mk(batch * gm.numelA, F32 if gm.a_f32 else T)
    Bm = mk(batch * gm.numelB, F32 if gm.b_f32 else T)
    C0 = mk(batch * gm.numelC, F32 if gm.c_f32 else T)
    return A, Bm, C0


def pab_gemm_cases():
    cases = []
    for hw, Cn in GEMM_SHAPES:
        for name, make in B_.GEMMS.items():
            gm = make(hw, Cn)
            for T in FWD_DTYPES:
                if T == F16 and name not in FWD_SETS:
                    continue
                for accum in (0, 1):
                    # accum = 1 once per C storage type: S (f32 scratch) and dbottom (T), at the shape with tails
                    if accum and not (hw == 20 and name in ('S', 'dbottom') and T != F16):
                        continue
                    for exact in (True, False):
                        g = R.gen(_seed('pab_gemm', hw, Cn, name, NAME[T], accum, exact))
                        A, Bm, C0 = _gemm_operands(gm, GEMM_BATCH, T, g, exact)
                        TC = F32 if gm.c_f32 else T
                        outs = dict(C=(C0.shape, TC, C0 if accum else None))
                        call = lambda B, t, gm=gm, accum=accum, T=T: B.pab_gemm(gm, t['A'], t['B'], t['C'], GEMM_BATCH, accum, CODE[T])      # noqa: E731
                        cid = f'pab_gemm-{name}-hw{hw}-C{Cn}-{"accum" if accum else "store"}-{NAME[T]}'
                        if exact:
                            cases.append(Case(cid.replace('pab_gemm-', 'pab_gemm-exact-'), T, dict(A=A, B=Bm), outs, call,
                                              refs=lambda gm=gm, A=A, Bm=Bm, C0=C0, accum=accum: dict(C=BR.pab_gemm(gm, GEMM_BATCH, A, Bm, C0 if accum else None)[0])))
                        else:
                            def check(t, gm=gm, A=A, Bm=Bm, C0=C0, accum=accum, T=T, name=name):
                                ref, sa = BR.pab_gemm(gm, GEMM_BATCH, A, Bm, C0 if accum else None)
                                _ratio(f'pab_gemm {name}', T, t['C'], ref, R.bound_r(ref, sa, gm.K + accum, None if gm.c_f32 else T))
                            cases.append(Case(cid, T, dict(A=A, B=Bm), outs, call, check=check))
    return cases


# =============================================================================================== pab_softmax
SOFTMAX_N = (256, 1296, 81)


def pab_softmax_cases():
    cases = []
    batch = 2
    for n in SOFTMAX_N:
        for T in TRAIN_DTYPES:      # float32 scratch whatever the dtype: the door must take both
            g = R.gen(_seed('pab_softmax', n, NAME[T]))
            fwd = lambda B, t, T=T: B.pab_softmax_fwd(t['S'], CODE[T])      # noqa: E731
            bwd = lambda B, t, T=T: B.pab_softmax_bwd(t['dP'], t['P'], CODE[T])      # noqa: E731
            if n == 256:
                # ---- Rule X twins: all entries equal -> P = 2^-8 exactly; uniform P and dyadic dP -> exact
                S0 = torch.stack([torch.full((n,), 3.25), torch.full((n,), -7.0)])
                cases.append(Case(f'pab_softmax_fwd-exact-n{n}-{NAME[T]}', T, {}, dict(S=(S0.shape, F32, S0)), fwd,
                                  refs=lambda S0=S0: dict(S=BR.pab_softmax_fwd(S0))))
                Pu = torch.full((batch, n), 2.0 ** -8)
                dPx = R.dyadic((batch, n), F32, g)
                cases.append(Case(f'pab_softmax_bwd-exact-n{n}-{NAME[T]}', T, dict(P=Pu), dict(dP=(dPx.shape, F32, dPx)), bwd,
                                  refs=lambda Pu=Pu, dPx=dPx: dict(dP=BR.pab_softmax_bwd(dPx, Pu)[0], P=R.d(Pu))))
            for kind, S0 in (('gauss', R.normal((batch, n), F32, g, 2.0)), ('spread', (torch.rand(batch, n, generator=g, dtype=torch.float64) * 400 - 200).to(F32))):
                def check_fwd(t, S0=S0, n=n, kind=kind):
                    ref = BR.pab_softmax_fwd(S0)
                    yard = torch.softmax(S0, dim=1)
                    R.assert_transcendental(t['S'], ref, yard, R.bound_e(ref, ref, BR.SOFTMAX_K, F32), f'pab_softmax_fwd {kind}', F32)
                    tot = t['S'].double().sum(1)
                    assert bool(((tot - 1).abs() <= n * R.EPS32).all()), f'an image sums to {tot.tolist()}'
                cases.append(Case(f'pab_softmax_fwd-{kind}-n{n}-{NAME[T]}', T, {}, dict(S=(S0.shape, F32, S0)), fwd, check=check_fwd))
            Pg = torch.softmax(R.normal((batch, n), F32, g, 2.0).double(), dim=1).to(F32)
            dPg = R.normal((batch, n), F32, g)

            def check_bwd(t, Pg=Pg, dPg=dPg, T=T):
                ref, mag = BR.pab_softmax_bwd(dPg, Pg)
                _ratio('pab_softmax_bwd dS', T, t['dP'], ref, R.bound_e(ref, mag, BR.SOFTMAX_BWD_K, F32))
                _bits_equal(t['P'], Pg, 'P after the backward')
            cases.append(Case(f'pab_softmax_bwd-n{n}-{NAME[T]}', T, dict(P=Pg), dict(dP=(dPg.shape, F32, dPg)), bwd, check=check_bwd))
    return cases


# =============================================================================================== pab_mix
PAB_MIX_SHAPES = ((2, 6, 8), (2, 20, 24))


def pab_mix_cases():
    cases = []
    for shape in PAB_MIX_SHAPES:
        N, HW, Cn = shape
        for T in FWD_DTYPES:
            g = R.gen(_seed('pab_mix', shape, NAME[T]))
            x, M = R.dyadic(shape, T, g), R.dyadic((N, HW * Cn), F32, g)
            cases.append(Case(f'pab_mix_fwd-{N}x{HW}x{Cn}-{NAME[T]}', T, dict(x=x, M=M), dict(y=(shape, T, None)),
                              lambda B, t: B.pab_mix_fwd(t['x'], t['M'], t['y']), refs=lambda x=x, M=M: dict(y=BR.pab_mix_fwd(x, M)[0])))
            if T == F16:
                continue
            dy = R.normal(shape, T, g)
            cases.append(Case(f'pab_mix_bwd-{N}x{HW}x{Cn}-{NAME[T]}', T, dict(dy=dy), dict(dM=((N, HW * Cn), F32, None)),
                              lambda B, t: B.pab_mix_bwd(t['dy'], t['dM']), refs=lambda dy=dy: dict(dM=BR.pab_mix_bwd(dy))))
    return cases


# =============================================================================================== the PAB chain
PAB_CHAIN = (2, 4, 5, 24)


def pab_chain_inputs(T):
    N, h, w, Cn = PAB_CHAIN
    hw = h * w
    g = R.gen(_seed('pab_chain', NAME[T]))
    return dict(x=R.normal((N, hw, Cn), T, g), center=R.normal((N, hw, 64), T, g, 0.25), top=R.normal((N, hw, 64), T, g, 0.25),
                bottom=R.normal((N, hw, Cn), T, g), dy=R.normal((N, hw, Cn), T, g))


def pab_chain_grads(i, dtype, T):
    leaf = lambda t: t.detach().clone().to(dtype).requires_grad_(True)      # noqa: E731
    c, tp, bt = leaf(i['center']), leaf(i['top']), leaf(i['bottom'])
    y, S, P, M = BR.pab_torch(i['x'], c, tp, bt, dtype)
    (y * i['dy'].to(dtype)).sum().backward()
    out = dict(y=y.detach(), dcenter=c.grad, dtop=tp.grad, dbottom=bt.grad)
    if dtype == torch.float32 and T != torch.float32:
        out = {k: v.to(T).to(dtype) for k, v in out.items()}
    return out


def pab_chain_cases():
    cases = []
    N, h, w, Cn = PAB_CHAIN
    hw = h * w
    G = {k: f(hw, Cn) for k, f in B_.GEMMS.items()}
    for T in TRAIN_DTYPES:
        i = pab_chain_inputs(T)
        outs = dict(S=((N, hw * hw), F32, None), P=((N, hw * hw), F32, None), M=((N, hw * Cn), F32, None), y=((N, hw, Cn), T, None),
                    dM=((N, hw * Cn), F32, None), dPraw=((N, hw * hw), F32, None), dP=((N, hw * hw), F32, None), dbottom=((N, hw, Cn), T, None),
                    dcenter=((N, hw, 64), T, None), dtop=((N, hw, 64), T, None))

        def call(B, t, T=T):
            dt = CODE[T]
            # forward, as plan_forward.cpp OP_PAB (S is kept beside P so that the softmax can be judged on its own input)
            B.pab_gemm(G['S'], t['center'], t['top'], t['S'], N, 0, dt)
            t['P'].copy_(t['S'])
            B.pab_softmax_fwd(t['P'], dt)
            B.pab_gemm(G['M'], t['P'], t['bottom'], t['M'], N, 0, dt)
            B.pab_mix_fwd(t['x'], t['M'], t['y'])
            # backward, as plan_backward.cpp OP_PAB
            B.pab_mix_bwd(t['dy'], t['dM'])
            B.pab_gemm(G['dP'], t['dM'], t['bottom'], t['dPraw'], N, 0, dt)
            B.pab_gemm(G['dbottom'], t['P'], t['dM'], t['dbottom'], N, 0, dt)
            t['dP'].copy_(t['dPraw'])
            B.pab_softmax_bwd(t['dP'], t['P'], dt)
            B.pab_gemm(G['dcenter'], t['dP'], t['top'], t['dcenter'], N, 0, dt)
            B.pab_gemm(G['dtop'], t['dP'], t['center'], t['dtop'], N, 0, dt)

        def check(t, T=T, i=i):
            _finite(t, list(outs))

            def gemm(name, A, Bm, got):
                ref, sa = BR.pab_gemm(G[name], N, A, Bm)
                _ratio(f'pab_chain {name}', T, got, ref, R.bound_r(ref, sa, G[name].K, None if G[name].c_f32 else T))
            gemm('S', i['center'], i['top'], t['S'])
            ref = BR.pab_softmax_fwd(t['S'])
            R.assert_transcendental(t['P'], ref, torch.softmax(t['S'], dim=1), R.bound_e(ref, ref, BR.SOFTMAX_K, F32), 'pab_chain softmax', T)
            gemm('M', t['P'], i['bottom'], t['M'])
            ref, mag = BR.pab_mix_fwd(i['x'], t['M'])
            _ratio('pab_chain y', T, t['y'], ref, R.bound_e(ref, mag, 1 + 2, T))
            R.assert_exact(t['dM'], BR.pab_mix_bwd(i['dy']), 'pab_chain dM')
            gemm('dP', t['dM'], i['bottom'], t['dPraw'])
            gemm('dbottom', t['P'], t['dM'], t['dbottom'])
            ref, mag = BR.pab_softmax_bwd(t['dPraw'], t['P'])
            _ratio('pab_chain dS', T, t['dP'], ref, R.bound_e(ref, mag, BR.SOFTMAX_BWD_K, F32))
            gemm('dcenter', t['dP'], i['top'], t['dcenter'])
            gemm('dtop', t['dP'], i['center'], t['dtop'])
            # end to end against float64 autograd of the torch PAB, by the yardstick rule of the pyramid backward
            r64, y32 = pab_chain_grads(i, torch.float64, T), pab_chain_grads(i, torch.float32, T)
            for k in sorted(r64):
                BR.yardstick_check(t[k], r64[k], y32[k], f'pab_chain-{k}-autograd', NAME[T])
        cases.append(Case(f'pab_chain-{NAME[T]}', T, {k: v for k, v in i.items()}, outs, call, check=check))
    return cases


FAMILIES = dict(maxpool2=maxpool2_cases, fpa_in=fpa_in_cases, fpa_pyr_fwd=fpa_pyr_fwd_cases, fpa_pyr_bwd=fpa_pyr_bwd_cases, fpa_mix=fpa_mix_cases,
                fpa_chain=fpa_chain_cases, pab_gemm=pab_gemm_cases, pab_softmax=pab_softmax_cases, pab_mix=pab_mix_cases, pab_chain=pab_chain_cases)
