"""The cases of the single-op sweep tests: inputs, the launcher call, and how the result is judged.

A Case is built on the CPU (inputs, float64 references) and run by tests/test_gpu_sweeps.py, which copies the inputs
into guarded device buffers, makes the call and hands CPU copies of every tensor to `check`.  A Rule X case gives `refs`
(a function -> {tensor name: reference}) instead: the result must equal each reference rounded once, bit for bit, and
tests/test_sweeps.py evaluates `refs` in float32 and in float64 on the CPU and asserts that the two agree, which proves
that the inputs are exact before a GPU sees them.  Tensors of `outs` start as NaN (init None) or from given values.
"""
import torch

import sweep_ref as R
from sweep_ref import d

F32, BF16, F16 = torch.float32, torch.bfloat16, torch.float16
TRAIN = (F32, BF16)
ALL = (F32, BF16, F16)
NAME = R.DTYPE_NAMES


class Case:
    def __init__(self, id, dtype, ins, outs, call, refs=None, check=None):
        self.id, self.dtype, self.ins, self.outs, self.call, self.refs, self.check = id, dtype, ins, outs, call, refs, check
        assert (refs is None) != (check is None)

    def __repr__(self):
        return self.id


def _c1(dtype):
    return 4 if dtype == F32 else 8       # one vector


def _seed(*parts):
    h = 0
    for p in parts:
        for ch in str(p):
            h = (h * 131 + ord(ch)) % 2147483647
    return h


def _stat_outs(Cn, names=('scale', 'shift', 'mean', 'rstd')):
    return {n: ((Cn,), F32, None) for n in names}


def _scratch_outs():
    return {'part': ((R_PART,), torch.float64, None), 'counters': ((64,), torch.int32, torch.zeros(64, dtype=torch.int32))}


R_PART = 2 * 16384


# =============================================================================================== bn_finalize_train
def _slab_with_totals(rows, tot, g, step):
    """[rows, C] multiples of `step` whose column sums are `tot` (float64 exact)."""
    Cn = tot.numel()
    part = torch.randint(-3, 4, (rows, Cn), generator=g).to(torch.float64) * step
    part[rows - 1] = tot - part[:rows - 1].sum(0)
    return part


def bn_finalize_train_cases():
    out = []
    # Rule X: every slab_cpb class (rows 1 / 7 -> 32 channels per block, 513 -> 16, 2049 -> 8, 6145 -> 4), C = 2240 (70 blocks of 32),
    # and rows = 131075 with C = 16: slab_groups = 2, the ticket-counter path.  count 1 and 2: unbiased = var and 2 var, both exact.
    for rows, Cn, count in ((1, 8, 1), (7, 40, 2), (7, 2240, 1), (513, 2240, 2), (2049, 8, 2), (6145, 40, 2), (131075, 16, 2)):
        g = R.gen(_seed('fin', rows, Cn))
        m = torch.randint(-2, 4, (Cn,), generator=g).to(torch.float64)
        v = torch.pow(4.0, torch.randint(-1, 3, (Cn,), generator=g).to(torch.float64))     # var in {1/4, 1, 4, 16}: rstd a power of two (eps = 0)
        slab = torch.stack([_slab_with_totals(rows, m * count, g, 1.0), _slab_with_totals(rows, (v + m * m) * count, g, 0.5)], -1).to(F32)
        ins = dict(slab=slab, gamma=R.pow2((Cn,), g), beta=R.ints((Cn,), g))
        rm0, rv0 = R.ints((Cn,), g), R.ints((Cn,), g, 0, 4)
        outs = dict(_stat_outs(Cn), running_mean=((Cn,), F32, rm0), running_var=((Cn,), F32, rv0), **_scratch_outs())

        def call(S, t, count=count):
            S.bn_finalize_train(t['slab'], count, t['gamma'], t['beta'], t['running_mean'], t['running_var'], 0.25, 0.0, t['scale'], t['shift'],
                                t['mean'], t['rstd'], t['part'], t['counters'])

        def refs(ins=ins, rm0=rm0, rv0=rv0, count=count):
            return R.bn_finalize_train(ins['slab'], count, ins['gamma'], ins['beta'], rm0, rv0, 0.25, 0.0)
        out.append(Case(f'bn_finalize_train-X-rows{rows}-C{Cn}-count{count}', F32, ins, outs, call, refs=refs))
    # rounded: partial sums of real data; mean and the running statistics by Rule E (double arithmetic, rounded once; the running update is
    # two float products and a sum: k = 3 + 2), rstd / scale / shift by Rule T
    for rows, Cn in ((513, 40), (2049, 8)):
        g = R.gen(_seed('finT', rows, Cn))
        x = torch.randn(rows, 16, Cn, generator=g, dtype=torch.float64) * 1.5 + 0.5
        slab = torch.stack([x.sum(1), (x * x).sum(1)], -1).to(F32)
        count = rows * 16
        ins = dict(slab=slab, gamma=R.normal((Cn,), F32, g), beta=R.normal((Cn,), F32, g))
        rm0, rv0 = R.normal((Cn,), F32, g), R.normal((Cn,), F32, g).abs()
        outs = dict(_stat_outs(Cn), running_mean=((Cn,), F32, rm0), running_var=((Cn,), F32, rv0), **_scratch_outs())

        def call(S, t, count=count):
            S.bn_finalize_train(t['slab'], count, t['gamma'], t['beta'], t['running_mean'], t['running_var'], 0.1, 1e-5, t['scale'], t['shift'],
                                t['mean'], t['rstd'], t['part'], t['counters'])

        def check(tc, ins=ins, rm0=rm0, rv0=rv0, count=count, tag=f'bn_finalize_train-rows{rows}'):
            args = (ins['slab'], count, ins['gamma'], ins['beta'], rm0, rv0, 0.1, 1e-5)
            ref = R.bn_finalize_train(*args)
            with R.as_float32():
                yard = R.bn_finalize_train(*args)
            _check_stats(tc, ref, yard, d(rm0), d(rv0), 0.1, tag)
        out.append(Case(f'bn_finalize_train-T-rows{rows}-C{Cn}', F32, ins, outs, call, check=check))
    return out


def _check_stats(tc, ref, yard, rm0, rv0, momentum, tag):
    R.assert_within(tc['mean'], ref['mean'], R.bound_e(ref['mean'], ref['mean'].abs(), 2, F32), tag + ' mean')
    R.assert_within(tc['running_mean'], ref['running_mean'],
                    R.bound_e(ref['running_mean'], (1 - momentum) * rm0.abs() + momentum * ref['mean'].abs(), 5, F32), tag + ' running_mean')
    unb = (ref['running_var'] - (1 - momentum) * rv0) / momentum
    R.assert_within(tc['running_var'], ref['running_var'], R.bound_e(ref['running_var'], (1 - momentum) * rv0.abs() + momentum * unb.abs(), 5, F32),
                    tag + ' running_var')
    # rstd: one divide and one square root (+ 2); scale: * gamma; shift: beta - mean * scale
    R.assert_transcendental(tc['rstd'], ref['rstd'], yard['rstd'], R.bound_e(ref['rstd'], ref['rstd'].abs(), 4, F32), tag + ' rstd', F32)
    R.assert_transcendental(tc['scale'], ref['scale'], yard['scale'], R.bound_e(ref['scale'], ref['scale'].abs(), 5, F32), tag + ' scale', F32)
    smag = (ref['shift'] + ref['mean'] * ref['scale']).abs() + (ref['mean'] * ref['scale']).abs()
    R.assert_transcendental(tc['shift'], ref['shift'], yard['shift'], R.bound_e(ref['shift'], smag, 7, F32), tag + ' shift', F32)


# =============================================================================================== bn_finalize_small
def bn_finalize_small_cases():
    out = []
    for dtype in TRAIN:
        for count, Cn in ((1, 8), (1024, 40), (1024, 8), (2, 40)):      # Rule X: count 1 (var 0, eps 1/4: rstd 2) and even counts (mean +- dev, eps 0)
            g = R.gen(_seed('small', count, Cn, dtype))
            m = torch.randint(-2, 4, (Cn,), generator=g).to(torch.float64)
            if count == 1:
                y, eps = m.view(1, Cn).clone(), 0.25
            else:
                dev = torch.pow(2.0, torch.randint(-1, 3, (Cn,), generator=g).to(torch.float64))
                sign = torch.stack([(torch.randperm(count, generator=g) % 2).to(torch.float64) * 2 - 1 for _ in range(Cn)], 1)
                y, eps = m + sign * dev, 0.0
            ins = dict(y=y.to(dtype), gamma=R.pow2((Cn,), g), beta=R.ints((Cn,), g))
            rm0, rv0 = R.ints((Cn,), g), R.ints((Cn,), g, 0, 4)
            exact_rv = count <= 2      # sum of squared deviations / (count - 1): exact only then
            outs = dict(_stat_outs(Cn), running_mean=((Cn,), F32, rm0), running_var=((Cn,), F32, rv0))

            def call(S, t, eps=eps):
                S.bn_finalize_small(t['y'], t['gamma'], t['beta'], t['running_mean'], t['running_var'], 0.25, eps, t['scale'], t['shift'], t['mean'], t['rstd'])

            def refs(ins=ins, rm0=rm0, rv0=rv0, eps=eps, exact_rv=exact_rv):
                r = R.bn_finalize_small(ins['y'], ins['gamma'], ins['beta'], rm0, rv0, 0.25, eps)
                if not exact_rv:
                    del r['running_var']
                return r
            out.append(Case(f'bn_finalize_small-X-{NAME[dtype]}-count{count}-C{Cn}', dtype, ins, outs, call, refs=refs))
        for count, Cn in ((1, 40), (31, 40), (129, 8), (1024, 40)):
            g = R.gen(_seed('smallT', count, Cn, dtype))
            ins = dict(y=R.normal((count, Cn), dtype, g, 1.5), gamma=R.normal((Cn,), F32, g), beta=R.normal((Cn,), F32, g))
            rm0, rv0 = R.normal((Cn,), F32, g), R.normal((Cn,), F32, g).abs()
            outs = dict(_stat_outs(Cn), running_mean=((Cn,), F32, rm0), running_var=((Cn,), F32, rv0))

            def call(S, t):
                S.bn_finalize_small(t['y'], t['gamma'], t['beta'], t['running_mean'], t['running_var'], 0.1, 1e-5, t['scale'], t['shift'], t['mean'], t['rstd'])

            def check(tc, ins=ins, rm0=rm0, rv0=rv0, tag=f'bn_finalize_small-{NAME[dtype]}-count{count}'):
                args = (ins['y'], ins['gamma'], ins['beta'], rm0, rv0, 0.1, 1e-5)
                ref = R.bn_finalize_small(*args)
                with R.as_float32():
                    yard = R.bn_finalize_small(*args)
                _check_stats(tc, ref, yard, d(rm0), d(rv0), 0.1, tag)
            out.append(Case(f'bn_finalize_small-T-{NAME[dtype]}-count{count}-C{Cn}', dtype, ins, outs, call, check=check))
    return out


# =============================================================================================== bn_finalize_eval / frozen
def bn_finalize_eval_cases():
    out = []
    for frozen in (False, True):
        names = ('scale', 'shift', 'mean', 'rstd') if frozen else ('scale', 'shift')
        op = 'bn_finalize_frozen' if frozen else 'bn_finalize_eval'

        def call(S, t, frozen=frozen, eps=0.25):
            if frozen:
                S.bn_finalize_frozen(t['gamma'], t['beta'], t['rm'], t['rv'], eps, t['scale'], t['shift'], t['mean'], t['rstd'], t['coef'])
            else:
                S.bn_finalize_eval(t['gamma'], t['beta'], t['rm'], t['rv'], eps, t['scale'], t['shift'])
        for Cn in (8, 300, 2240):      # 300: a partly filled last block of 256
            g = R.gen(_seed(op, Cn))
            rv = torch.pow(4.0, torch.randint(0, 3, (Cn,), generator=g).to(torch.float64)) - 0.25      # rv + 1/4 in {1, 4, 16}
            ins = dict(gamma=R.pow2((Cn,), g), beta=R.ints((Cn,), g), rm=R.ints((Cn,), g), rv=rv.to(F32))
            outs = _stat_outs(Cn, names)
            if frozen:
                outs['coef'] = ((Cn, 2), F32, None)

            def refs(ins=ins, frozen=frozen, names=names):
                r = R.bn_finalize_eval(ins['gamma'], ins['beta'], ins['rm'], ins['rv'], 0.25)
                r = {k: r[k] for k in names}
                if frozen:
                    r['coef'] = torch.zeros(ins['gamma'].numel(), 2, dtype=R.REF_DTYPE[0])      # coef must be 0
                return r
            out.append(Case(f'{op}-X-C{Cn}', F32, ins, outs, call, refs=refs))
        Cn = 304
        g = R.gen(_seed(op, 'T'))
        ins = dict(gamma=R.normal((Cn,), F32, g), beta=R.normal((Cn,), F32, g), rm=R.normal((Cn,), F32, g), rv=R.normal((Cn,), F32, g).abs() + 0.01)
        outs = _stat_outs(Cn, names)
        if frozen:
            outs['coef'] = ((Cn, 2), F32, None)

        def callT(S, t, call=call):
            call(S, t, eps=1e-5)

        def check(tc, ins=ins, frozen=frozen, names=names, op=op):
            args = (ins['gamma'], ins['beta'], ins['rm'], ins['rv'], 1e-5)
            ref = R.bn_finalize_eval(*args)
            with R.as_float32():
                yard = R.bn_finalize_eval(*args)
            mags = dict(scale=(ref['scale'].abs(), 4), rstd=(ref['rstd'].abs(), 5), mean=(ref['mean'].abs(), 2),
                        shift=(d(ins['beta']).abs() + (d(ins['rm']) * ref['scale']).abs(), 6))     # add, sqrt, divide (, divide | multiply, subtract) + 2
            for k in names:
                R.assert_transcendental(tc[k], ref[k], yard[k], R.bound_e(ref[k], mags[k][0], mags[k][1], F32), f'{op} {k}', F32)
            if frozen:
                R.assert_exact(tc['coef'], torch.zeros(Cn, 2, dtype=torch.float64), f'{op} coef')
        out.append(Case(f'{op}-T-C{Cn}', F32, ins, outs, callT, check=check))
    return out


# =============================================================================================== bn_act
# (scale, res, rscale, post, relu, maskbits): training forwards save the mask bits of their ReLU, residual blocks add the shortcut raw or
# through the downsample BatchNorm, decoder blocks add a skip after the activation, eval forwards come with BatchNorm folded (no scale)
BN_ACT_FORMS = ((1, 0, 0, 0, 1, 1), (1, 1, 0, 0, 1, 1), (1, 1, 1, 0, 1, 1), (1, 0, 0, 1, 1, 0), (0, 0, 0, 0, 1, 0), (0, 1, 0, 0, 1, 0),
                (1, 0, 0, 0, 0, 0), (1, 0, 0, 1, 0, 1), (1, 1, 1, 1, 1, 1))


def _bn_act_case(dtype, npix, Cn, form, exact, tag=''):
    sc, rs, rsc, po, relu, mb = form
    g = R.gen(_seed('bn_act', dtype, npix, Cn, form, exact))
    val = (lambda shape: R.dyadic(shape, dtype, g)) if exact else (lambda shape: R.normal(shape, dtype, g))
    par = (lambda: R.pow2((Cn,), g)) if exact else (lambda: R.normal((Cn,), F32, g))
    shf = (lambda: R.ints((Cn,), g) * 0.25) if exact else (lambda: R.normal((Cn,), F32, g))
    ins = dict(y=val((npix, Cn)), scale=par() if sc else None, shift=shf() if sc else None, res=val((npix, Cn)) if rs else None,
               rscale=par() if rsc else None, rshift=shf() if rsc else None, post=val((npix, Cn)) if po else None)
    vec = R.VEC[dtype]
    outs = dict(out=((npix, Cn), dtype, None))
    if mb:
        outs['maskbits'] = ((npix, Cn // vec), torch.uint8, None)

    def call(S, t, relu=relu):
        S.bn_act(t['y'], t['out'], t['scale'], t['shift'], t['res'], t['rscale'], t['rshift'], t['post'], relu=bool(relu), maskbits=t.get('maskbits'))

    def ref(ins=ins, relu=relu):
        return R.bn_act(ins['y'], ins['scale'], ins['shift'], ins['res'], ins['rscale'], ins['rshift'], ins['post'], relu=bool(relu))
    name = f'bn_act-{"X" if exact else "E"}-{NAME[dtype]}-npix{npix}-C{Cn}-form{"".join(map(str, form))}{tag}'
    if exact:
        def refs(ref=ref, mb=mb, vec=vec):
            x, _ = ref()
            r = dict(out=x)
            if mb:
                r['maskbits'] = R.pack_mask(x > 0, vec)       # bits of the value BEFORE it is rounded to T (exact: the same set)
            return r
        return Case(name, dtype, ins, outs, call, refs=refs)

    def check(tc, ref=ref, mb=mb, vec=vec, dtype=dtype, name=name):
        x, mag = ref()
        bound = R.bound_e(x, mag, R.BN_ACT_K, dtype)
        R.assert_within(tc['out'], x, bound, name)
        if mb:      # the bit follows the float value before storage: certain wherever |x| exceeds the float error bound
            sure = x.abs() > R.BN_ACT_K * R.EPS32 * mag
            got = tc['maskbits']
            want = R.pack_mask(x > 0, vec)
            gb = _unpack_mask(got, vec)
            assert want.shape == got.shape and torch.equal(gb[sure], (x > 0)[sure]), name + ' mask bits'
            assert bool(sure.any()), name + ' mask bits: nothing judged'
    return Case(name, dtype, ins, outs, call, check=check)


def _unpack_mask(m, vec):
    npix, nv = m.shape
    return ((m.to(torch.int64).unsqueeze(-1) >> torch.arange(vec)) & 1).bool().view(npix, nv * vec)


def bn_act_cases():
    out = []
    for dtype in ALL:
        for form in BN_ACT_FORMS:
            out.append(_bn_act_case(dtype, 7, 48, form, True))
        for npix, Cn in ((1, _c1(dtype)), (300, 24), (37, 304), (5, 2240), (3, 64)):
            out.append(_bn_act_case(dtype, npix, Cn, BN_ACT_FORMS[8], True))
        out.append(_bn_act_case(dtype, 300, 48, BN_ACT_FORMS[8], False))
        out.append(_bn_act_case(dtype, 37, 304, BN_ACT_FORMS[2], False))
    for dtype in ALL:      # more than 8192 x 256 vectors: the grid-stride loop's second trip and its tail (vpc 3: a grid of 8190 blocks)
        npix = 8192 * 256 // 3 + 1001
        out.append(_bn_act_case(dtype, npix, 3 * R.VEC[dtype], BN_ACT_FORMS[1], True, tag='-secondtrip'))
    return out


# =============================================================================================== BatchNorm backward
def _plan_rows(npix, Cn, dtype):
    vpc = Cn // R.VEC[dtype]
    tpv = 1 if vpc >= 256 else 256 // vpc
    return min(1024, (npix + tpv - 1) // tpv), tpv


def _bwd_inputs(dtype, npix, Cn, mask, exact, g):
    """g, y, per-channel vectors; mask source for mode 2 (out or bits)."""
    if exact:
        gg, y = R.dyadic((npix, Cn), dtype, g, -4, 4), R.dyadic((npix, Cn), dtype, g)
        mean, rstd, gamma, beta = R.ints((Cn,), g, -2, 2), R.pow2((Cn,), g, -1, 1, signed=False), R.pow2((Cn,), g, -1, 1), R.ints((Cn,), g, -2, 2) * 0.5
    else:
        gg, y = R.normal((npix, Cn), dtype, g), R.normal((npix, Cn), dtype, g, 1.5)
        mean, rstd = R.normal((Cn,), F32, g, 0.5), (R.normal((Cn,), F32, g).abs() + 0.5)
        gamma, beta = R.normal((Cn,), F32, g), R.normal((Cn,), F32, g, 0.5)
    scale = (gamma.double() * rstd.double()).to(F32)
    shift = (beta.double() - mean.double() * scale.double()).to(F32)
    return dict(g=gg, y=y, mean=mean, rstd=rstd, gamma=gamma, scale=scale, shift=shift)


def _mask_source(ins, kind, dtype, g):
    """kind: 0 none, 1 recomputed, 2 from `out`, 3 from mask bits.  -> (mask mode, maskpos or None)"""
    npix, Cn = ins['y'].shape
    ins['out'] = None
    ins['maskbits'] = None
    if kind == 2:
        ins['out'] = R.dyadic((npix, Cn), dtype, g, -3, 3)       # (zeros abound: out > 0 is false there)
        return 2, None
    if kind == 3:
        pos = torch.randint(0, 2, (npix, Cn), generator=g).bool()
        ins['maskbits'] = R.pack_mask(pos, R.VEC[dtype])
        return 2, pos
    return kind, None


def _dz(ins, mask, pos):
    return R.bn_bwd_mask(ins['g'], ins['y'], mask, ins['scale'], ins['shift'], ins['out'], pos)


def bn_bwd_reduce_cases():
    out = []
    for dtype in TRAIN:
        wide = (2048, 2240) if dtype == BF16 else (1024, 1152, 2240)       # vpc 256 / 280 | 256 / 288 / 560
        shapes = [(1, _c1(dtype), 0, 1), (1101, _c1(dtype), 0, 1), (1101, 24, 0, 1), (1101, 48, 0, 2), (1101, 64, 0, 3), (530, 304, 0, 1)]
        shapes += [(1101, 64, 3, k) for k in (0, 1, 2, 3)]                # rows = 3: a workgroup walks several pixel groups
        shapes += [(1030, Cn, 0, 1) for Cn in wide] + [(1030, wide[-1], 3, 3), (5, wide[-1], 0, 2)]
        for npix, Cn, rows, kind in shapes:
            for exact in (True, False):
                if not exact and (Cn in wide[:-1] or npix <= 5):
                    continue
                # a term of sum dz xhat is formed by three rounded operations: Rule R is asked of rows that add at least 8 terms
                if not exact and int(torch.bincount(R.bn_bwd_row_of_pixel(npix, rows or _plan_rows(npix, Cn, dtype)[0], _plan_rows(npix, Cn, dtype)[1])).min()) < 8:
                    continue
                g = R.gen(_seed('reduce', dtype, npix, Cn, rows, kind, exact))
                ins = _bwd_inputs(dtype, npix, Cn, kind, exact, g)
                mask, pos = _mask_source(ins, kind, dtype, g)
                prow, tpv = _plan_rows(npix, Cn, dtype)
                nrows = rows or prow
                outs = dict(slab=((nrows, Cn, 2), F32, None))

                def call(S, t, mask=mask):
                    S.bn_bwd_reduce(t['g'], t['y'], t['scale'], t['shift'], t['mean'], t['rstd'], t['slab'], mask=mask, out=t['out'], maskbits=t['maskbits'])

                def ref(ins=ins, mask=mask, pos=pos, nrows=nrows, tpv=tpv):
                    return R.bn_bwd_reduce(_dz(ins, mask, pos), ins['y'], ins['mean'], ins['rstd'], nrows, tpv)
                name = f'bn_bwd_reduce-{"X" if exact else "R"}-{NAME[dtype]}-npix{npix}-C{Cn}-rows{nrows}-mask{kind}'
                if exact:
                    out.append(Case(name, dtype, ins, outs, call, refs=lambda ref=ref: dict(slab=ref()[0])))
                else:
                    def check(tc, ref=ref, name=name):
                        slab, sa, n = ref()
                        R.assert_within(tc['slab'], slab, R.bound_r(slab, sa, n.view(-1, 1, 1)), name)
                    out.append(Case(name, dtype, ins, outs, call, check=check))
    return out


def bn_bwd_finalize_cases():
    out = []
    for rows, Cn in ((1, 8), (3, 64), (1024, 2240), (1024, 1152), (2049, 40)):
        g = R.gen(_seed('bwdfin', rows, Cn))
        npix = 2048
        slab = torch.stack([_slab_with_totals(rows, torch.randint(-64, 65, (Cn,), generator=g).to(torch.float64) * 8, g, 0.25),
                            _slab_with_totals(rows, torch.randint(-64, 65, (Cn,), generator=g).to(torch.float64) * 8, g, 0.25)], -1).to(F32)
        dg0, db0 = R.ints((Cn,), g), R.ints((Cn,), g)
        ins = dict(slab=slab)
        outs = dict(dgamma=((Cn,), F32, dg0), dbeta=((Cn,), F32, db0), coef=((Cn, 2), F32, None), **_scratch_outs())

        def call(S, t, npix=npix):
            S.bn_bwd_finalize(t['slab'], npix, t['dgamma'], t['dbeta'], t['coef'], t['part'], t['counters'])

        def refs(slab=slab, dg0=dg0, db0=db0, npix=npix):
            s = d(slab).sum(0)
            return dict(dbeta=d(db0) + s[:, 0], dgamma=d(dg0) + s[:, 1], coef=s / npix)
        out.append(Case(f'bn_bwd_finalize-X-rows{rows}-C{Cn}', F32, ins, outs, call, refs=refs))
    return out


RES_FORMS = (None, 'store', 'accum')


def _res_out(outs, ins, res, dtype, g):
    npix, Cn = ins['y'].shape
    r0 = None
    if res == 'store':
        outs['res_grad'] = ((npix, Cn), dtype, None)
    elif res == 'accum':
        r0 = R.dyadic((npix, Cn), dtype, g, -4, 4)
        outs['res_grad'] = ((npix, Cn), dtype, r0)
    return r0


def bn_bwd_apply_cases():
    out = []
    for dtype in TRAIN:
        wide = (2048, 2240) if dtype == BF16 else (1152, 2240)
        shapes = [(1, _c1(dtype), 0, None), (1101, 24, 1, None), (1101, 48, 2, 'store'), (530, 304, 3, 'accum')]
        shapes += [(1101, 64, k, r) for k in (0, 1, 2, 3) for r in RES_FORMS]
        shapes += [(70, Cn, 1, 'store') for Cn in wide]
        for npix, Cn, kind, res in shapes:
            for exact in (True, False):
                if not exact and (npix == 1 or (Cn == 64 and res == 'store')):
                    continue
                out.append(_apply_case(dtype, npix, Cn, kind, res, exact))
    # more than 4 x 8192 x 256 vectors (bf16): the four-deep unroll runs full, then clamped.  Exact inputs: the float32 CPU evaluation IS the reference
    out.append(_apply_case(BF16, 4 * 8192 * 256 + 8192 * 256 + 77, 8, 1, None, True, big=True))
    return out


def _apply_case(dtype, npix, Cn, kind, res, exact, big=False):
    g = R.gen(_seed('apply', dtype, npix, Cn, kind, res, exact))
    ins = _bwd_inputs(dtype, npix, Cn, kind, exact, g)
    mask, pos = _mask_source(ins, kind, dtype, g)
    ins['coef'] = (R.ints((Cn, 2), g) * 0.25) if exact else R.normal((Cn, 2), F32, g, 0.3)
    outs = {}
    r0 = _res_out(outs, ins, res, dtype, g)
    # dy aliases g, as the plan calls it: the gradient tensor is rewritten in place

    def call(S, t, mask=mask, res=res):
        S.bn_bwd_apply(t['g'], t['y'], t['scale'], t['shift'], t['mean'], t['rstd'], t['gamma'], t['coef'], t['g'], mask=mask, out=t['out'],
                       maskbits=t['maskbits'], res_grad=t.get('res_grad'), res_store=res == 'store')

    def ref(ins=ins, mask=mask, pos=pos):
        dz = _dz(ins, mask, pos)
        return dz, R.bn_bwd_apply(dz, ins['y'], ins['mean'], ins['rstd'], ins['gamma'], ins['coef'])
    name = f'bn_bwd_apply-{"X" if exact else "E"}-{NAME[dtype]}-npix{npix}-C{Cn}-mask{kind}-res{res}'
    if exact:
        def refs(ref=ref, res=res, r0=r0, big=big):
            if big:      # 84 M elements: one float32 pass (exact inputs make it the reference)
                with R.as_float32():
                    dz, (dy, _) = ref()
            else:
                dz, (dy, _) = ref()
            r = dict(g=dy)
            if res:
                r['res_grad'] = dz if res == 'store' else dz + d(r0)
            return r
        c = Case(name, dtype, ins, outs, call, refs=refs)
        c.big = big

        def sample_refs(stride=4099):      # every 4099th pixel of the big case: proves its inputs exact without a float64 pass over all of them
            sub = {k: (v[::stride] if torch.is_tensor(v) and v.dim() == 2 and v.shape[0] == npix else v) for k, v in ins.items()}
            dz = _dz(sub, mask, None if pos is None else pos[::stride])
            return dict(g=R.bn_bwd_apply(dz, sub['y'], sub['mean'], sub['rstd'], sub['gamma'], sub['coef'])[0])
        c.sample_refs = sample_refs
        return c

    def check(tc, ref=ref, res=res, r0=r0, dtype=dtype, name=name):
        dz, (dy, mag) = ref()
        R.assert_within(tc['g'], dy, R.bound_e(dy, mag, R.BN_APPLY_K, dtype), name)
        if res == 'store':
            R.assert_exact(tc['res_grad'], dz, name + ' res_grad')
        elif res == 'accum':      # one float sum, stored as T
            R.assert_within(tc['res_grad'], dz + d(r0), R.bound_e(dz + d(r0), dz.abs() + d(r0).abs(), 3, dtype), name + ' res_grad')
    return Case(name, dtype, ins, outs, call, check=check)


def bn_bwd_small_cases():
    out = []
    for dtype in TRAIN:
        shapes = [(1, 8, 0, None), (31, 40, 1, 'store'), (129, 40, 2, 'accum'), (1024, 8, 3, None), (1024, 40, 1, 'accum'), (64, 72, 1, None)]
        shapes += [(64, 40, k, 'store') for k in (0, 2, 3)]
        for npix, Cn, kind, res in shapes:
            g = R.gen(_seed('bsmall', dtype, npix, Cn, kind, res))
            exact = npix & (npix - 1) == 0                    # the means divide by npix: exact for powers of two
            ins = _bwd_inputs(dtype, npix, Cn, kind, exact, g)
            mask, pos = _mask_source(ins, kind, dtype, g)
            dg0, db0 = R.ints((Cn,), g), R.ints((Cn,), g)
            outs = dict(dgamma=((Cn,), F32, dg0), dbeta=((Cn,), F32, db0), coef=((Cn, 2), F32, None))
            r0 = _res_out(outs, ins, res, dtype, g)

            def call(S, t, mask=mask, res=res):
                S.bn_bwd_small(t['g'], t['y'], t['scale'], t['shift'], t['mean'], t['rstd'], t['gamma'], t['dgamma'], t['dbeta'], t['coef'], t['g'],
                               mask=mask, out=t['out'], maskbits=t['maskbits'], res_grad=t.get('res_grad'), res_store=res == 'store')

            def ref(ins=ins, mask=mask, pos=pos, dg0=dg0, db0=db0, npix=npix):
                dz = _dz(ins, mask, pos)
                slab, sa, _ = R.bn_bwd_reduce(dz, ins['y'], ins['mean'], ins['rstd'], 1, 1)
                coef = slab[0] / npix
                dy, mag = R.bn_bwd_apply(dz, ins['y'], ins['mean'], ins['rstd'], ins['gamma'], coef)
                return dz, slab[0], sa[0], coef, dy, mag
            name = f'bn_bwd_small-{"X" if exact else "E"}-{NAME[dtype]}-npix{npix}-C{Cn}-mask{kind}-res{res}'
            if exact:
                def refs(ref=ref, res=res, r0=r0, dg0=dg0, db0=db0):
                    dz, s, _, coef, dy, _ = ref()
                    r = dict(g=dy, coef=coef, dbeta=d(db0) + s[:, 0], dgamma=d(dg0) + s[:, 1])
                    if res:
                        r['res_grad'] = dz if res == 'store' else dz + d(r0)
                    return r
                out.append(Case(name, dtype, ins, outs, call, refs=refs))
            else:
                def check(tc, ref=ref, res=res, r0=r0, dg0=dg0, db0=db0, dtype=dtype, name=name, npix=npix):
                    # the kernel sums and applies in double and rounds once: everything by Rule E on the float64 values; dy with k = 0 + 2
                    dz, s, sa, coef, dy, mag = ref()
                    R.assert_within(tc['coef'], coef, R.bound_e(coef, coef.abs(), 2, F32), name + ' coef')       # one conversion
                    for key, col, x0 in (('dbeta', 0, d(db0)), ('dgamma', 1, d(dg0))):       # conversion of the total, one float sum: k = 2 + 2
                        R.assert_within(tc[key], x0 + s[:, col], R.bound_e(x0 + s[:, col], x0.abs() + s[:, col].abs(), 4, F32), f'{name} {key}')
                    R.assert_within(tc['g'], dy, R.bound_e(dy, mag, 2, dtype), name + ' dy')
                    if res == 'store':
                        R.assert_exact(tc['res_grad'], dz, name + ' res_grad')
                    elif res == 'accum':
                        R.assert_within(tc['res_grad'], dz + d(r0), R.bound_e(dz + d(r0), dz.abs() + d(r0).abs(), 3, dtype), name + ' res_grad')
                out.append(Case(name, dtype, ins, outs, call, check=check))
    return out


def bn_bwd_chain_cases():
    """reduce -> finalize -> apply as plan_backward.cpp chains them (dy aliases g), Rule X end to end: 512 pixels (the means are exact)."""
    out = []
    for dtype in TRAIN:
        wide = (2048, 2240) if dtype == BF16 else (1152, 2240)
        for Cn, kind, res, rows in ((64, 3, 'store', 0), (24, 1, None, 3), (304, 2, 'accum', 0)) + tuple((c, 1, None, 0) for c in wide):
            npix = 512
            g = R.gen(_seed('chain', dtype, Cn, kind, res))
            ins = _bwd_inputs(dtype, npix, Cn, kind, True, g)
            mask, pos = _mask_source(ins, kind, dtype, g)
            prow, tpv = _plan_rows(npix, Cn, dtype)
            nrows = rows or prow
            dg0, db0 = R.ints((Cn,), g), R.ints((Cn,), g)
            outs = dict(slab=((nrows, Cn, 2), F32, None), dgamma=((Cn,), F32, dg0), dbeta=((Cn,), F32, db0), coef=((Cn, 2), F32, None), **_scratch_outs())
            r0 = _res_out(outs, ins, res, dtype, g)

            def call(S, t, mask=mask, res=res, npix=npix):
                S.bn_bwd_reduce(t['g'], t['y'], t['scale'], t['shift'], t['mean'], t['rstd'], t['slab'], mask=mask, out=t['out'], maskbits=t['maskbits'])
                S.bn_bwd_finalize(t['slab'], npix, t['dgamma'], t['dbeta'], t['coef'], t['part'], t['counters'])
                S.bn_bwd_apply(t['g'], t['y'], t['scale'], t['shift'], t['mean'], t['rstd'], t['gamma'], t['coef'], t['g'], mask=mask, out=t['out'],
                               maskbits=t['maskbits'], res_grad=t.get('res_grad'), res_store=res == 'store')

            def refs(ins=ins, mask=mask, pos=pos, nrows=nrows, tpv=tpv, res=res, r0=r0, dg0=dg0, db0=db0, npix=npix):
                dz = _dz(ins, mask, pos)
                slab, _, _ = R.bn_bwd_reduce(dz, ins['y'], ins['mean'], ins['rstd'], nrows, tpv)
                s = slab.sum(0)
                dy, _ = R.bn_bwd_apply(dz, ins['y'], ins['mean'], ins['rstd'], ins['gamma'], s / npix)
                r = dict(slab=slab, coef=s / npix, dbeta=d(db0) + s[:, 0], dgamma=d(dg0) + s[:, 1], g=dy)
                if res:
                    r['res_grad'] = dz if res == 'store' else dz + d(r0)
                return r
            out.append(Case(f'bn_bwd_chain-X-{NAME[dtype]}-C{Cn}-rows{nrows}-mask{kind}-res{res}', dtype, ins, outs, call, refs=refs))
    return out


# =============================================================================================== gradient plumbing, plain sweeps
def plumbing_cases():
    out = []
    for dtype in ALL:
        train = dtype != F16
        v = R.VEC[dtype]
        for exact in (True, False):
            X = 'X' if exact else 'E'
            g = R.gen(_seed('plumb', dtype, exact))
            val = (lambda *shape: R.dyadic(shape, dtype, g)) if exact else (lambda *shape: R.normal(shape, dtype, g))
            N, H, W, Cn = 2, 3, 5, 3 * v       # odd H and W, vpc 3

            def judge(name, key, ref_fn, mag_fn, k, exact=exact, dtype=dtype):
                if exact:
                    return dict(refs=lambda: {key: ref_fn()})
                return dict(check=lambda tc: R.assert_within(tc[key], ref_fn(), R.bound_e(ref_fn(), mag_fn(), k, dtype), name))
            if train:
                for store in (True, False):
                    for masked in (True, False):
                        ins = dict(g=val(N * H * W, Cn), m=R.dyadic((N * H * W, Cn), dtype, g, -2, 2) if masked else None)
                        d0 = None if store else val(N * H * W, Cn)
                        name = f'masked_accum-{X}-{NAME[dtype]}-store{int(store)}-mask{int(masked)}'

                        def gm(ins=ins):
                            return d(ins['g']) if ins['m'] is None else torch.where(d(ins['m']) > 0, d(ins['g']), torch.zeros_like(d(ins['g'])))
                        out.append(Case(name, dtype, ins, dict(dst=((N * H * W, Cn), dtype, d0)),
                                        lambda S, t, store=store: S.masked_accum(t['dst'], t['g'], t['m'], store=store),
                                        **judge(name, 'dst', lambda gm=gm, d0=d0: gm() + (0 if d0 is None else d(d0)),
                                                lambda gm=gm, d0=d0: gm().abs() + (0 if d0 is None else d(d0).abs()), 3)))
                    ins = dict(src=val(N, 2 * H, 2 * W, Cn))
                    d0 = None if store else val(N, H, W, Cn)
                    name = f'pool2x2_accum-{X}-{NAME[dtype]}-store{int(store)}'
                    out.append(Case(name, dtype, ins, dict(dst=((N, H, W, Cn), dtype, d0)),
                                    lambda S, t, store=store: S.pool2x2_accum(t['dst'], t['src'], store=store),
                                    **judge(name, 'dst', lambda ins=ins, d0=d0: R.pool2x2(ins['src']) + (0 if d0 is None else d(d0)),
                                            lambda ins=ins, d0=d0: R.pool2x2(ins['src'].abs()) + (0 if d0 is None else d(d0).abs()), 4 + 2)))
            if exact:
                ins = dict(x=val(N, H, W, Cn))
                out.append(Case(f'up2_fill-X-{NAME[dtype]}', dtype, ins, dict(out=((N, 2 * H, 2 * W, Cn), dtype, None)),
                                lambda S, t: S.up2_fill(t['x'], t['out']), refs=lambda ins=ins: dict(out=R.up2(ins['x']))))
                ins = dict(x=val(N * H * W, Cn), m=R.dyadic((N * H * W, Cn), dtype, g, -2, 2))
                out.append(Case(f'relu-X-{NAME[dtype]}-fwd', dtype, ins, dict(out=((N * H * W, Cn), dtype, None)),
                                lambda S, t: S.relu(t['x'], t['out']), refs=lambda ins=ins: dict(out=d(ins['x']).clamp_min(0))))
                out.append(Case(f'relu-X-{NAME[dtype]}-masked', dtype, ins, dict(out=((N * H * W, Cn), dtype, None)),
                                lambda S, t: S.relu(t['x'], t['out'], mask=t['m']),
                                refs=lambda ins=ins: dict(out=torch.where(d(ins['m']) > 0, d(ins['x']), torch.zeros_like(d(ins['x']))))))
            ins = dict(a=val(N * H * W, Cn), b=val(N * H * W, Cn))
            name = f'add2-{X}-{NAME[dtype]}'
            out.append(Case(name, dtype, ins, dict(out=((N * H * W, Cn), dtype, None)), lambda S, t: S.add2(t['a'], t['b'], t['out']),
                            **judge(name, 'out', lambda ins=ins: d(ins['a']) + d(ins['b']), lambda ins=ins: d(ins['a']).abs() + d(ins['b']).abs(), 3)))
            for keep in (True, False):        # mscale 2 (p = 0.5) in the exact form, 1 / 0.8 otherwise
                ms = 2.0 if exact else 1.25
                ins = dict(x=val(N * H * W, Cn), keep=torch.randint(0, 2, (N * H * W, Cn), generator=g).to(F32) if keep else None)
                name = f'drop_elem-{X}-{NAME[dtype]}-keep{int(keep)}'

                def de(ins=ins, ms=ms):
                    return d(ins['x']) if ins['keep'] is None else d(ins['x']) * d(ins['keep']) * ms
                out.append(Case(name, dtype, ins, dict(out=((N * H * W, Cn), dtype, None)),
                                lambda S, t, ms=ms: S.drop_elem(t['x'], t['out'], keep=t['keep'], mscale=ms),
                                **judge(name, 'out', de, lambda de=de: de().abs(), 2 + 2)))
                ms = 2.0 if exact else 1.25
                m = torch.randint(0, 2, (N, Cn), generator=g).to(F32) if keep else None
                ins = dict(a0=val(N, H * W, Cn), a1=val(N, H * W, Cn), a2=val(N, H * W, Cn), a3=val(N, H * W, Cn), m=m)
                name = f'merge_drop-{X}-{NAME[dtype]}-m{int(keep)}'

                def md(ins=ins, ms=ms, absolute=False):
                    f = (lambda t: d(t).abs()) if absolute else d
                    s = f(ins['a0']) + f(ins['a1']) + f(ins['a2']) + f(ins['a3'])
                    return s if ins['m'] is None else s * (d(ins['m']) * ms).unsqueeze(1)
                out.append(Case(name, dtype, ins, dict(out=((N, H * W, Cn), dtype, None)),
                                lambda S, t, ms=ms: S.merge_drop(t['a0'], t['a1'], t['a2'], t['a3'], t['out'], m=t['m'], mscale=ms),
                                **judge(name, 'out', md, lambda md=md: md(absolute=True), 5 + 2)))
                ins = dict(gout=val(N, H * W, Cn), m=m)
                name = f'drop_bwd-{X}-{NAME[dtype]}-m{int(keep)}'

                def db(ins=ins, ms=ms):
                    return d(ins['gout']) if ins['m'] is None else d(ins['gout']) * (d(ins['m']) * ms).unsqueeze(1)
                out.append(Case(name, dtype, ins, dict(gin=((N, H * W, Cn), dtype, None)),
                                lambda S, t, ms=ms: S.drop_bwd(t['gout'], t['gin'], m=t['m'], mscale=ms),
                                **judge(name, 'gin', db, lambda db=db: db().abs(), 2 + 2)))
    return out


# =============================================================================================== channel_sum, tensor_stats
def channel_sum_cases():
    """out[c] += sum over pixels (float atomics between workgroups: arrival order; exact inputs make every order give the same sum)."""
    out = []
    for dtype in TRAIN:
        v = R.VEC[dtype]
        for Cn, Cstride, npix in ((v, 2 * v, 1), (48, 64, 4500), (256 * v, 256 * v + v, 70),       # 256 vectors: the vector kernel's widest (bf16 C = 2048, f32 C = 1024)
                                   (1, 8, 3000), (3, 8, 3000), (3, 3, 77)):
            for exact in (True, False):
                g = R.gen(_seed('csum', dtype, Cn, Cstride, npix, exact))
                gt = R.dyadic((npix, Cstride), dtype, g) if exact else R.normal((npix, Cstride), dtype, g)
                o0 = R.ints((Cn,), g)
                name = f'channel_sum-{"X" if exact else "R"}-{NAME[dtype]}-C{Cn}-stride{Cstride}-npix{npix}'

                det = exact and npix in (4500, 3000)       # deterministic mode (one workgroup) on the many-pixel cases as well

                def call(S, t, Cn=Cn):
                    S.channel_sum(t['g'], Cn, t['out'])

                def call_det(S, t, Cn=Cn):
                    import os
                    S.L.lib().octseg_set_deterministic(1)
                    try:
                        S.channel_sum(t['g'], Cn, t['out'])
                    finally:
                        S.L.lib().octseg_set_deterministic(1 if os.environ.get('OCTSEG_DETERMINISTIC') else 0)
                if det:
                    out.append(Case(name + '-deterministic', dtype, dict(g=gt), dict(out=((Cn,), F32, o0)), call_det,
                                    refs=lambda gt=gt, o0=o0, Cn=Cn: dict(out=d(o0) + d(gt)[:, :Cn].sum(0))))
                if exact:
                    out.append(Case(name, dtype, dict(g=gt), dict(out=((Cn,), F32, o0)), call,
                                    refs=lambda gt=gt, o0=o0, Cn=Cn: dict(out=d(o0) + d(gt)[:, :Cn].sum(0))))
                else:
                    def check(tc, gt=gt, o0=o0, Cn=Cn, npix=npix, name=name):
                        ref = d(o0) + d(gt)[:, :Cn].sum(0)
                        R.assert_within(tc['out'], ref, R.bound_r(ref, d(o0).abs() + d(gt)[:, :Cn].abs().sum(0), npix + 1), name)
                    out.append(Case(name, dtype, dict(g=gt), dict(out=((Cn,), F32, o0)), call, check=check))
    return out


def tensor_stats_cases():
    out = []
    for dtype in TRAIN:
        for npix, Cn, rows in ((1, _c1(dtype), 1), (700, 48, 5), (300, 2240, 3), (300, 1624, 512), (64, 2048, 2)):
            for exact in (True, False):
                g = R.gen(_seed('tstats', dtype, npix, Cn, rows, exact))
                y = R.dyadic((npix, Cn), dtype, g) if exact else R.normal((npix, Cn), dtype, g)
                vtot = Cn // R.VEC[dtype]
                name = f'tensor_stats-{"X" if exact else "R"}-{NAME[dtype]}-npix{npix}-C{Cn}-rows{rows}'
                if not exact and npix // rows < 8:
                    continue

                def ref(y=y, npix=npix, Cn=Cn, rows=rows, vtot=vtot, dtype=dtype):
                    """pixel p goes to row (p / tpv) mod rows, tpv per chunk of <= 256 channel vectors"""
                    slab = torch.zeros(rows, Cn, 2, dtype=R.REF_DTYPE[0])
                    sa = torch.zeros_like(slab)
                    n = torch.zeros(rows, Cn, 1, dtype=R.REF_DTYPE[0])
                    yy = d(y)
                    for cv0 in range(0, vtot, 256):
                        vpc = min(256, vtot - cv0)
                        c0, c1 = cv0 * R.VEC[dtype], (cv0 + vpc) * R.VEC[dtype]
                        row = R.tensor_stats_row(npix, rows, 256 // vpc)
                        slab[:, c0:c1, 0].index_add_(0, row, yy[:, c0:c1])
                        slab[:, c0:c1, 1].index_add_(0, row, yy[:, c0:c1] ** 2)
                        sa[:, c0:c1, 0].index_add_(0, row, yy[:, c0:c1].abs())
                        n[:, c0:c1, 0].index_add_(0, row, torch.ones(npix, c1 - c0, dtype=R.REF_DTYPE[0]))
                    sa[..., 1] = slab[..., 1]
                    return slab, sa, n

                def call(S, t):
                    S.tensor_stats(t['y'], t['slab'])
                if exact:
                    out.append(Case(name, dtype, dict(y=y), dict(slab=((rows, Cn, 2), F32, None)), call, refs=lambda ref=ref: dict(slab=ref()[0])))
                else:
                    def check(tc, ref=ref, name=name):
                        slab, sa, n = ref()
                        R.assert_within(tc['slab'], slab, R.bound_r(slab, sa, n), name)       # (a square is formed and added by ONE fma)
                    out.append(Case(name, dtype, dict(y=y), dict(slab=((rows, Cn, 2), F32, None)), call, check=check))
    return out


# =============================================================================================== maxpool
def maxpool_cases():
    """Values are multiples of 0.5 (ties abound: the first maximum in scan order wins); one channel vector all negative, -inf sprinkled in."""
    out = []
    for dtype in ALL:
        for N, H, W, Cn in ((1, 2, 2, _c1(dtype)), (2, 6, 10, 24), (1, 4, 4, 304)):
            g = R.gen(_seed('maxpool', dtype, H, W, Cn))
            x = R.dyadic((N, H, W, Cn), dtype, g, -3, 3, 0.5)
            x[..., :R.VEC[dtype] // 2] = -x[..., :R.VEC[dtype] // 2].abs() - 0.5          # all-negative windows
            x[torch.rand(N, H, W, Cn, generator=g) < 0.1] = float('-inf')
            x[0, 0, 0, -1] = float('-inf')
            x[0, 0, 1, -1] = float('-inf')
            x[0, 1, 0, -1] = float('-inf')
            x[0, 1, 1, -1] = float('-inf')                                                  # a window of -inf only: the maximum is -inf
            OH, OW = H // 2, W // 2
            gout = R.dyadic((N, OH, OW, Cn), dtype, g)
            ins = dict(x=x)
            out.append(Case(f'maxpool_fwd-X-{NAME[dtype]}-{H}x{W}-C{Cn}', dtype, ins,
                            dict(out=((N, OH, OW, Cn), dtype, None), idx=((N, OH, OW, Cn), torch.uint8, None)),
                            lambda S, t: S.maxpool_fwd(t['x'], t['out'], t['idx']),
                            refs=lambda x=x: dict(zip(('out', 'idx'), R.maxpool_fwd(x)))))
            out.append(Case(f'maxpool_fwd-X-{NAME[dtype]}-{H}x{W}-C{Cn}-noidx', dtype, ins, dict(out=((N, OH, OW, Cn), dtype, None)),
                            lambda S, t: S.maxpool_fwd(t['x'], t['out'], None), refs=lambda x=x: dict(out=R.maxpool_fwd(x)[0])))
            if dtype == F16:
                continue
            for store in (True, False):
                g0 = None if store else R.dyadic((N, H, W, Cn), dtype, g)

                def call(S, t, store=store):      # the saved indices round-trip: forward, then the backward from its own idx
                    S.maxpool_fwd(t['x'], t['out'], t['idx'])
                    S.maxpool_bwd_idx(t['idx'], t['gout'], t['gin'], store=store)

                def refs(x=x, gout=gout, g0=g0, H=H, W=W):
                    o, idx = R.maxpool_fwd(x)
                    return dict(out=o, idx=idx, gin=R.maxpool_bwd(idx, gout, H, W) + (0 if g0 is None else d(g0)))
                out.append(Case(f'maxpool_bwd_idx-X-{NAME[dtype]}-{H}x{W}-C{Cn}-store{int(store)}', dtype, dict(x=x, gout=gout),
                                dict(out=((N, OH, OW, Cn), dtype, None), idx=((N, OH, OW, Cn), torch.uint8, None), gin=((N, H, W, Cn), dtype, g0)),
                                call, refs=refs))
    return out


# =============================================================================================== bilinear resize and adjoints
RESIZES = (((1, 1), (5, 7)), ((3, 5), (6, 10)), ((2, 3), (7, 4)), ((6, 6), (22, 22)), ((5, 4), (5, 4)))


def bilinear_cases():
    out = []
    for dtype in ALL:
        for (IH, IW), (OH, OW) in RESIZES:
            N, Cn = 2, 3 * R.VEC[dtype]
            g = R.gen(_seed('bilinear', dtype, IH, IW, OH, OW))
            x = R.normal((N, IH, IW, Cn), dtype, g)
            name = f'bilinear_resize-E-{NAME[dtype]}-{IH}x{IW}-to-{OH}x{OW}'

            def check(tc, x=x, OH=OH, OW=OW, dtype=dtype, name=name):
                def one():
                    ref, mag = R.bilinear_resize(x, OH, OW)
                    R.assert_within(tc['out'], ref, R.bound_e(ref, mag, R.BILINEAR_K, dtype), name)
                R.either_weights(one)
            out.append(Case(name, dtype, dict(x=x), dict(out=((N, OH, OW, Cn), dtype, None)), lambda S, t: S.bilinear_resize(t['x'], t['out']), check=check))
            if dtype == F16:
                continue
            go = R.normal((N, OH, OW, Cn), dtype, g)
            name = f'bilinear_resize_adjoint-R-{NAME[dtype]}-{IH}x{IW}-from-{OH}x{OW}'

            def check_adj(tc, go=go, IH=IH, IW=IW, dtype=dtype, name=name):
                def one():
                    ref, sa, nt = R.bilinear_adjoint(go, IH, IW, float_products=True)
                    R.assert_within(tc['gin'], ref, R.bound_r(ref, sa, nt.view(1, IH, IW, 1), dtype), name)
                R.either_weights(one)
            out.append(Case(name, dtype, dict(gout=go), dict(gin=((N, IH, IW, Cn), dtype, None)),
                            lambda S, t: S.bilinear_resize_adjoint(t['gout'], t['gin']), check=check_adj))
        # Rule X: size pairs whose scale (in - 1) / (out - 1) is 1, 1/2 or 1/4 -- every weight is dyadic, so dyadic maps resample exactly
        for (IH, IW), (OH, OW) in (((5, 4), (5, 4)), ((3, 5), (5, 9)), ((2, 3), (5, 9)), ((1, 1), (5, 7))):
            N, Cn = 2, 3 * R.VEC[dtype]
            g = R.gen(_seed('bilinearX', dtype, IH, IW, OH, OW))
            xe = R.dyadic((N, IH, IW, Cn), dtype, g)
            out.append(Case(f'bilinear_resize-X-{NAME[dtype]}-{IH}x{IW}-to-{OH}x{OW}', dtype, dict(x=xe), dict(out=((N, OH, OW, Cn), dtype, None)),
                            lambda S, t: S.bilinear_resize(t['x'], t['out']), refs=lambda xe=xe, OH=OH, OW=OW: dict(out=R.bilinear_resize(xe, OH, OW)[0])))
            if dtype != F16:
                ge = R.dyadic((N, OH, OW, Cn), dtype, g)
                out.append(Case(f'bilinear_resize_adjoint-X-{NAME[dtype]}-{IH}x{IW}-from-{OH}x{OW}', dtype, dict(gout=ge), dict(gin=((N, IH, IW, Cn), dtype, None)),
                                lambda S, t: S.bilinear_resize_adjoint(t['gout'], t['gin']),
                                refs=lambda ge=ge, IH=IH, IW=IW: dict(gin=R.bilinear_adjoint(ge, IH, IW)[0])))
        if dtype == F16:
            continue
        for up, H, W in ((2, 3, 5), (4, 3, 5), (2, 1, 3), (4, 1, 3), (4, 1, 1)):       # a one-pixel axis: scale 0, every output reads that pixel
            N, Cn = 2, 3 * R.VEC[dtype]
            g = R.gen(_seed('biladj', dtype, up, H, W))
            go = R.normal((N, H * up, W * up, Cn), dtype, g)
            name = f'bilinear_adjoint-R-{NAME[dtype]}-{H}x{W}-up{up}'

            def check_up(tc, go=go, H=H, W=W, up=up, dtype=dtype, name=name):
                def one():
                    ref, sa, nt = R.bilinear_adjoint(go, H, W, float_products=True)
                    R.assert_within(tc['gin'], ref, R.bound_r(ref, sa, nt.view(1, H, W, 1), dtype), name)
                R.either_weights(one)
            out.append(Case(name, dtype, dict(gout=go), dict(gin=((N, H, W, Cn), dtype, None)),
                            lambda S, t, up=up: S.bilinear_adjoint(t['gout'], t['gin'], up), check=check_up))
    # 260 x 260 source pixels = 67600 workgroups: grid.y x grid.z = 33800 x 2.  Identity size: the adjoint of the identity is the identity (Rule X)
    g = R.gen(_seed('biladj-big'))
    go = R.dyadic((1, 260, 260, 8), BF16, g)
    c = Case('bilinear_resize_adjoint-X-bf16-260x260-identity', BF16, dict(gout=go), dict(gin=((1, 260, 260, 8), BF16, None)),
             lambda S, t: S.bilinear_resize_adjoint(t['gout'], t['gin']), refs=lambda go=go: dict(gin=d(go)))
    out.append(c)
    # the same grid with a real gather: 519 x 519 -> 260 x 260 has scale 1/2, so every weight is dyadic (Rule X) and each workgroup walks 3 x 3 outputs
    go2 = R.dyadic((1, 519, 519, 8), BF16, g, -4, 4)
    out.append(Case('bilinear_resize_adjoint-X-bf16-260x260-from-519x519', BF16, dict(gout=go2), dict(gin=((1, 260, 260, 8), BF16, None)),
                    lambda S, t: S.bilinear_resize_adjoint(t['gout'], t['gin']), refs=lambda go2=go2: dict(gin=R.bilinear_adjoint(go2, 260, 260)[0])))
    return out


# =============================================================================================== adaptive average pooling
def bin_mean_cases():
    out = []
    for dtype in ALL:
        for N, H, W, Cn, k in ((2, 22, 22, 3 * R.VEC[dtype], 1), (2, 22, 22, 48, 2), (2, 22, 22, 48, 3), (2, 22, 22, 304, 6), (1, 3, 5, 24, 6),
                               (8, 22, 22, 48, 6), (7, 22, 22, 48, 6), (29, 6, 6, 24, 3)):       # N k^2 = 288 | 252 | 261: both chunk widths
            g = R.gen(_seed('binmean', dtype, N, H, W, Cn, k))
            x = R.normal((N, H, W, Cn), dtype, g)
            name = f'bin_mean-R-{NAME[dtype]}-N{N}-{H}x{W}-C{Cn}-k{k}'

            def check(tc, x=x, k=k, dtype=dtype, name=name):
                ref, sa, cnt = R.bin_mean(x, k)
                R.assert_within(tc['out'], ref, R.bound_r(ref, sa, cnt.view(1, k, k, 1), dtype), name)       # cnt - 1 additions and the division
            out.append(Case(name, dtype, dict(x=x), dict(out=((N, k, k, Cn), dtype, None)), lambda S, t, k=k: S.bin_mean(t['x'], t['out'], k), check=check))
            if dtype == F16 or N > 2:
                continue
            for accum in (False, True):
                go = R.normal((N, k, k, Cn), dtype, g)
                g0 = R.normal((N, H, W, Cn), dtype, g) if accum else None
                name = f'bin_mean_bwd-R-{NAME[dtype]}-{H}x{W}-C{Cn}-k{k}-accum{int(accum)}'

                def check_b(tc, go=go, g0=g0, H=H, W=W, dtype=dtype, name=name):
                    ref, sa, nt = R.bin_mean_bwd(go, H, W)
                    if g0 is not None:
                        ref, sa = ref + d(g0), sa + d(g0).abs()
                    R.assert_within(tc['gin'], ref, R.bound_r(ref, sa, nt.view(1, H, W, 1) + (0 if g0 is None else 1), dtype), name)
                out.append(Case(name, dtype, dict(gout=go), dict(gin=((N, H, W, Cn), dtype, g0)),
                                lambda S, t, k=k, accum=accum: S.bin_mean_bwd(t['gout'], t['gin'], k, accum=accum), check=check_b))
        # Rule X: 16 x 16 maps, k = 2 / 4 (bins of 64 / 16 pixels: the division is exact)
        for k in (2, 4):
            g = R.gen(_seed('binmeanX', dtype, k))
            x = R.dyadic((2, 16, 16, 24), dtype, g)
            out.append(Case(f'bin_mean-X-{NAME[dtype]}-16x16-k{k}', dtype, dict(x=x), dict(out=((2, k, k, 24), dtype, None)),
                            lambda S, t, k=k: S.bin_mean(t['x'], t['out'], k), refs=lambda x=x, k=k: dict(out=R.bin_mean(x, k)[0])))
            if dtype != F16:
                go = R.dyadic((2, k, k, 24), dtype, g)
                out.append(Case(f'bin_mean_bwd-X-{NAME[dtype]}-16x16-k{k}', dtype, dict(gout=go), dict(gin=((2, 16, 16, 24), dtype, None)),
                                lambda S, t, k=k: S.bin_mean_bwd(t['gout'], t['gin'], k), refs=lambda go=go: dict(gin=R.bin_mean_bwd(go, 16, 16)[0])))
    return out


# =============================================================================================== per-image sums, broadcast, gates
def image_cases():
    out = []
    for dtype in ALL:
        for N, HW, Cn in ((3, 1, _c1(dtype)), (3, 63, 224), (3, 64, 2240), (3, 4097, 8), (3, 64, 224)):
            g = R.gen(_seed('image', dtype, HW, Cn))
            exact_ok = HW in (1, 64)
            for exact in ((True, False) if exact_ok else (False,)):
                X = 'X' if exact else 'R'
                x = R.dyadic((N, HW, Cn), dtype, g) if exact else R.normal((N, HW, Cn), dtype, g)
                name = f'image_sum-{X}-{NAME[dtype]}-HW{HW}-C{Cn}'
                if exact:
                    out.append(Case(name, dtype, dict(x=x), dict(out=((N, Cn), dtype, None)), lambda S, t, HW=HW: S.image_sum(t['x'], t['out'], div=float(HW)),
                                    refs=lambda x=x, HW=HW: dict(out=d(x).sum(1) / HW)))
                else:
                    def check(tc, x=x, HW=HW, dtype=dtype, name=name):
                        ref = d(x).sum(1) / HW
                        R.assert_within(tc['out'], ref, R.bound_r(ref, d(x).abs().sum(1) / HW, HW, dtype), name)
                    out.append(Case(name, dtype, dict(x=x), dict(out=((N, Cn), dtype, None)), lambda S, t, HW=HW: S.image_sum(t['x'], t['out'], div=float(HW)), check=check))
            if HW == 4097 and Cn == 8 or Cn == 224:
                for accum in (False, True):      # broadcast: Rule X (scale 1 / 4)
                    v = R.dyadic((N, Cn), dtype, g)
                    o0 = R.dyadic((N, HW, Cn), dtype, g) if accum else None
                    out.append(Case(f'image_bcast-X-{NAME[dtype]}-HW{HW}-C{Cn}-accum{int(accum)}', dtype, dict(v=v), dict(out=((N, HW, Cn), dtype, o0)),
                                    lambda S, t, accum=accum: S.image_bcast(t['v'], t['out'], scale=0.25, accum=accum),
                                    refs=lambda v=v, o0=o0, HW=HW: dict(out=(d(v) * 0.25).unsqueeze(1).expand(-1, HW, -1) + (0 if o0 is None else d(o0)))))
        for N, HW, Cn, two, accum in ((3, 1, _c1(dtype), False, False), (3, 63, 224, True, False), (3, 64, 2240, False, True), (3, 4097, 8, True, True)):
            g = R.gen(_seed('segate', dtype, HW, Cn))
            x, s = R.normal((N, HW, Cn), dtype, g), R.normal((N, Cn), dtype, g, 2.0)
            s2 = R.normal((N, Cn), dtype, g, 2.0) if two else None
            o0 = R.normal((N, HW, Cn), dtype, g) if accum else None
            name = f'se_gate-T-{NAME[dtype]}-HW{HW}-C{Cn}-two{int(two)}-accum{int(accum)}'

            def check(tc, x=x, s=s, s2=s2, o0=o0, dtype=dtype, name=name):
                ref, mag = R.se_gate(x, s, o0, s2)
                yard, _ = R.se_gate(x, s, o0, s2, f32=True)
                R.assert_transcendental(tc['out'], ref, yard.to(dtype), R.bound_e(ref, mag, R.SE_GATE_K + (2 if s2 is not None else 0), dtype), name, dtype)
            out.append(Case(name, dtype, dict(x=x, s=s, s2=s2), dict(out=((N, HW, Cn), dtype, o0)),
                            lambda S, t, accum=accum: S.se_gate(t['x'], t['s'], t['out'], accum=accum, s2=t['s2']), check=check))
            if dtype == F16:
                continue
            gg = R.normal((N, HW, Cn), dtype, g)
            shares = min(max(HW // 64, 1), 64)
            outs = dict(ds=((N, Cn), dtype, None), part=((N, shares, Cn), F32, None))
            if two:
                outs['ds2'] = ((N, Cn), dtype, None)
            name = f'se_dgate-T-{NAME[dtype]}-HW{HW}-C{Cn}-two{int(two)}'

            def check_d(tc, gg=gg, x=x, s=s, s2=s2, HW=HW, dtype=dtype, name=name):
                for key, sv in (('ds', s), ('ds2', s2)):
                    if sv is None:
                        continue
                    ref, mag = R.se_dgate(gg, x, sv)
                    yard, _ = R.se_dgate(gg, x, sv, f32=True)
                    R.assert_transcendental(tc[key], ref, yard.to(dtype), R.bound_r(ref, mag, HW, dtype), f'{name} {key}', dtype)
            out.append(Case(name, dtype, dict(g=gg, x=x, s=s, s2=s2), outs,
                            lambda S, t: S.se_dgate(t['g'], t['x'], t['s'], t['ds'], t['part'], s2=t['s2'], ds2=t.get('ds2')), check=check_d))
    return out


# =============================================================================================== re-arrangements
def rearrange_cases():
    out = []
    for dtype in ALL:
        g = R.gen(_seed('rearr', dtype))
        N, H, W, Cn = 2, 6, 10, 3 * R.VEC[dtype]
        x = R.dyadic((N, H, W, Cn), dtype, g)
        for accum in (False, True):
            c0 = R.dyadic((4 * N, H // 2, W // 2, Cn), dtype, g) if accum else None
            f0 = R.dyadic((N, H, W, Cn), dtype, g) if accum else None
            out.append(Case(f'parity_permute-X-{NAME[dtype]}-to_coarse-accum{int(accum)}', dtype, dict(x=x), dict(out=((4 * N, H // 2, W // 2, Cn), dtype, c0)),
                            lambda S, t, accum=accum: S.parity_permute(t['x'], t['out'], N, H, W, True, accum=accum),
                            refs=lambda c0=c0, x=x: dict(out=R.parity_to_coarse(d(x)) + (0 if c0 is None else d(c0)))))
            xc = R.parity_to_coarse(x)
            out.append(Case(f'parity_permute-X-{NAME[dtype]}-to_fine-accum{int(accum)}', dtype, dict(x=xc), dict(out=((N, H, W, Cn), dtype, f0)),
                            lambda S, t, accum=accum: S.parity_permute(t['x'], t['out'], N, H, W, False, accum=accum),
                            refs=lambda f0=f0, xc=xc: dict(out=R.parity_to_fine(d(xc)) + (0 if f0 is None else d(f0)))))
        for r in (2, 3):
            Hm, Wm = 7, 5         # neither a multiple of r: padding behind H and W
            xm = R.dyadic((N, Hm, Wm, Cn), dtype, g)
            _, _, MH, MW = R.mosaic_index(Hm, Wm, r)
            out.append(Case(f'mosaic-X-{NAME[dtype]}-r{r}-to_mosaic', dtype, dict(x=xm), dict(out=((N, MH, MW, Cn), dtype, None)),
                            lambda S, t, r=r: S.mosaic(t['x'], t['out'], N, Hm, Wm, r, True), refs=lambda xm=xm, r=r: dict(out=R.to_mosaic(d(xm), r))))
            mm = R.dyadic((N, MH, MW, Cn), dtype, g)
            for accum in (False, True):
                f0 = R.dyadic((N, Hm, Wm, Cn), dtype, g) if accum else None
                out.append(Case(f'mosaic-X-{NAME[dtype]}-r{r}-from_mosaic-accum{int(accum)}', dtype, dict(x=mm), dict(out=((N, Hm, Wm, Cn), dtype, f0)),
                                lambda S, t, r=r, accum=accum: S.mosaic(t['x'], t['out'], N, Hm, Wm, r, False, accum=accum),
                                refs=lambda mm=mm, r=r, f0=f0: dict(out=R.from_mosaic(d(mm), Hm, Wm, r) + (0 if f0 is None else d(f0)))))
    return out


# =============================================================================================== depthwise 3x3, CAM seed
def dw_cases():
    """8 x 8 maps: at dilation 12 only the centre tap is live.  in / out / weights are channel slices at non-zero offsets of wider tensors;
    the channels outside the output slice must stay untouched (they start as NaN in the store form)."""
    out = []
    for dtype in ALL:
        _dw_cases_of(dtype, out)
    _cam_seed_cases(out)
    return out


def _dw_cases_of(dtype, out):
    v = R.VEC[dtype]
    N, H, W, Cn = 2, 8, 8, 3 * v
    inC, ic0, outC, oc0, wC, wc0 = Cn + 2 * v, v, Cn + v, v, Cn + 8, 4
    for dil, flip, accum in ((1, 0, 0), (2, 1, 0), (12, 0, 1), (1, 1, 1), (2, 0, 0)):
        for exact in (True, False):
            g = R.gen(_seed('dw', dtype, dil, flip, accum, exact))
            x = R.dyadic((N, H, W, inC), dtype, g, -4, 4) if exact else R.normal((N, H, W, inC), dtype, g)
            w = (R.ints((9, wC), g) * 0.25) if exact else R.normal((9, wC), F32, g, 0.5)
            o0 = R.dyadic((N, H, W, outC), dtype, g, -4, 4) if exact else R.normal((N, H, W, outC), dtype, g)
            if not accum:
                o0[..., oc0:oc0 + Cn] = float('nan')       # the store form overwrites its slice and nothing else
            name = f'dw_conv-{"X" if exact else "R"}-{NAME[dtype]}-dil{dil}-flip{flip}-accum{accum}'

            def ref(x=x, w=w, o0=o0, dil=dil, flip=flip, accum=accum):
                r, sa = R.dw_conv(x[..., ic0:ic0 + Cn], w[:, wc0:wc0 + Cn], dil, bool(flip))
                full, fa = d(o0).clone(), d(o0).abs()
                full[..., oc0:oc0 + Cn] = r + (full[..., oc0:oc0 + Cn] if accum else 0)
                fa[..., oc0:oc0 + Cn] = sa + (fa[..., oc0:oc0 + Cn] if accum else 0)
                return full, fa

            def call(S, t, dil=dil, flip=flip, accum=accum):
                S.dw_conv(t['x'], ic0, t['out'], oc0, t['w'], wc0, Cn, dil, flip=bool(flip), accum=bool(accum))
            if exact:
                out.append(Case(name, dtype, dict(x=x, w=w), dict(out=((N, H, W, outC), dtype, o0)), call, refs=lambda ref=ref: dict(out=ref()[0])))
            else:
                def check(tc, ref=ref, dtype=dtype, name=name, accum=accum):
                    full, fa = ref()
                    R.assert_within(tc['out'], full, R.bound_r(full, fa, 9 + (1 if accum else 0), dtype), name)
                out.append(Case(name, dtype, dict(x=x, w=w), dict(out=((N, H, W, outC), dtype, o0)), call, check=check))
            if dtype == F16 or flip:
                continue
            go = R.dyadic((N, H, W, outC), dtype, g, -4, 4) if exact else R.normal((N, H, W, outC), dtype, g)
            dw0 = R.ints((9, wC), g)
            for det in ((False, True) if exact else (False,)):
                name = f'dw_wgrad-{"X" if exact else "R"}-{NAME[dtype]}-dil{dil}-det{int(det)}'

                def refw(x=x, go=go, dw0=dw0, dil=dil):
                    r, sa = R.dw_wgrad(x[..., ic0:ic0 + Cn], go[..., oc0:oc0 + Cn], dil)
                    full, fa = d(dw0).clone(), d(dw0).abs()
                    full[:, wc0:wc0 + Cn] += r
                    fa[:, wc0:wc0 + Cn] += sa
                    return full, fa

                def callw(S, t, dil=dil, det=det):
                    import os
                    if det:
                        S.L.lib().octseg_set_deterministic(1)
                    try:
                        S.dw_wgrad(t['x'], ic0, t['gout'], oc0, t['dw'], wc0, Cn, dil)
                    finally:
                        if det:
                            S.L.lib().octseg_set_deterministic(1 if os.environ.get('OCTSEG_DETERMINISTIC') else 0)
                if exact:
                    out.append(Case(name, dtype, dict(x=x, gout=go), dict(dw=((9, wC), F32, dw0)), callw, refs=lambda refw=refw: dict(dw=refw()[0])))
                else:
                    def checkw(tc, refw=refw, name=name):
                        full, fa = refw()
                        R.assert_within(tc['dw'], full, R.bound_r(full, fa, N * H * W + 1), name)
                    out.append(Case(name, dtype, dict(x=x, gout=go), dict(dw=((9, wC), F32, dw0)), callw, check=checkw))


def _cam_seed_cases(out):
    for dtype in TRAIN:      # the CAM seed: NCHW f32 -> NHWC T rows padded to CP channels; the padding must be exactly zero
        for B, Cn, HW, CP in ((2, 1, 300, 8), (1, 3, 77, 8), (2, 3, 1, 16), (1, 9, 260, 16)):
            g = R.gen(_seed('camseed', dtype, Cn, HW, CP))
            seed = R.normal((B, Cn, HW), F32, g)

            def refs(seed=seed, B=B, Cn=Cn, HW=HW, CP=CP, dtype=dtype):
                full = torch.zeros(B, HW, CP, dtype=R.REF_DTYPE[0])
                full[..., :Cn] = seed.to(dtype).to(R.REF_DTYPE[0]).permute(0, 2, 1)      # one rounding to T, nothing else
                return dict(out=full)
            out.append(Case(f'cam_seed-X-{NAME[dtype]}-C{Cn}-HW{HW}-CP{CP}', dtype, dict(seed=seed), dict(out=((B, HW, CP), dtype, None)),
                            lambda S, t: S.cam_seed(t['seed'], t['out']), refs=refs))



# =============================================================================================== EfficientNet sweeps, Dice gradient, GroupNorm
def _det_call(S, det, fn):
    import os
    if det:
        S.L.lib().octseg_set_deterministic(1)
    try:
        fn()
    finally:
        if det:
            S.L.lib().octseg_set_deterministic(1 if os.environ.get('OCTSEG_DETERMINISTIC') else 0)


def _dwg_of(dtype, K, stride, H, W, out):
    v = R.VEC[dtype]
    N, Cn = 2, 3 * v
    (OH, pt), (OW, pl) = R.tf_same(H, K, stride), R.tf_same(W, K, stride)
    assert pt == pl or True
    pad = pt      # square kernels on the maps below: the same top and left padding
    for exact in (True, False):
        g = R.gen(_seed('dwg', dtype, K, stride, H, W, exact))
        val = (lambda *sh: R.dyadic(sh, dtype, g, -4, 4)) if exact else (lambda *sh: R.normal(sh, dtype, g))
        x, go = val(N, H, W, Cn), val(N, OH, OW, Cn)
        w = (R.ints((K, K, Cn), g) * 0.25) if exact else R.normal((K, K, Cn), F32, g, 0.5)
        tag = f'{"X" if exact else "R"}-{NAME[dtype]}-K{K}-s{stride}-{H}x{W}'
        fwd = lambda x=x, w=w: R.dwg_fwd(x, w, OH, OW, K, stride, pad)
        call = lambda S, t: S.dwg_fwd(t['x'], t['out'], t['w'], K, stride, pad)
        if exact:
            out.append(Case('dwg_fwd-' + tag, dtype, dict(x=x, w=w), dict(out=((N, OH, OW, Cn), dtype, None)), call, refs=lambda fwd=fwd: dict(out=fwd()[0])))
        else:
            def check(tc, fwd=fwd, tag=tag):
                ref, sa = fwd()
                R.assert_within(tc['out'], ref, R.bound_r(ref, sa, K * K, dtype), 'dwg_fwd-' + tag)
            out.append(Case('dwg_fwd-' + tag, dtype, dict(x=x, w=w), dict(out=((N, OH, OW, Cn), dtype, None)), call, check=check))
        if dtype == F16:
            continue
        for accum in (False, True):
            g0 = val(N, H, W, Cn) if accum else None
            bwd = lambda go=go, w=w: R.dwg_bwd_data(go, w, H, W, K, stride, pad)
            callb = lambda S, t, accum=accum: S.dwg_bwd_data(t['gout'], t['gin'], t['w'], K, stride, pad, accum=accum)
            name = f'dwg_bwd_data-{tag}-accum{int(accum)}'
            if exact:
                out.append(Case(name, dtype, dict(gout=go, w=w), dict(gin=((N, H, W, Cn), dtype, g0)), callb,
                                refs=lambda bwd=bwd, g0=g0: dict(gin=bwd()[0] + (0 if g0 is None else d(g0)))))
            else:
                def checkb(tc, bwd=bwd, g0=g0, name=name):
                    ref, sa, nt = bwd()
                    if g0 is not None:
                        ref, sa, nt = ref + d(g0), sa + d(g0).abs(), nt + 1
                    R.assert_within(tc['gin'], ref, R.bound_r(ref, sa, nt.clamp_min(1).view(1, H, W, 1), dtype), name)
                out.append(Case(name, dtype, dict(gout=go, w=w), dict(gin=((N, H, W, Cn), dtype, g0)), callb, check=checkb))
        dw0 = R.ints((K, K, Cn), g)
        wg = lambda x=x, go=go: R.dwg_bwd_w(x, go, K, stride, pad)
        for det in ((False, True) if exact else (False,)):
            callw = lambda S, t, det=det: _det_call(S, det, lambda: S.dwg_bwd_w(t['x'], t['gout'], t['dw'], K, stride, pad))
            name = f'dwg_bwd_w-{tag}-det{int(det)}'
            if exact:
                out.append(Case(name, dtype, dict(x=x, gout=go), dict(dw=((K, K, Cn), F32, dw0)), callw, refs=lambda wg=wg, dw0=dw0: dict(dw=wg()[0] + d(dw0))))
            else:
                def checkw(tc, wg=wg, dw0=dw0, name=name):
                    ref, sa = wg()
                    R.assert_within(tc['dw'], ref + d(dw0), R.bound_r(ref, sa + d(dw0).abs(), N * OH * OW + 1), name)
                out.append(Case(name, dtype, dict(x=x, gout=go), dict(dw=((K, K, Cn), F32, dw0)), callw, check=checkw))


def dwg_cases():
    out = []
    for dtype in ALL:
        for K, stride, H, W in ((3, 1, 8, 8), (3, 2, 8, 8), (3, 2, 7, 7), (5, 1, 7, 7), (5, 2, 8, 8), (5, 2, 9, 9)):      # TF "same": even maps pad asymmetrically at stride 2
            _dwg_of(dtype, K, stride, H, W, out)
    return out


def _bnx_of(dtype, act, form, out):
    sc, ds, po = form
    N, hw, Cn = 3, 37, 3 * R.VEC[dtype]
    npix = N * hw
    exact = act == 0
    g = R.gen(_seed('bnx', dtype, act, form))
    val = (lambda *sh: R.dyadic(sh, dtype, g)) if exact else (lambda *sh: R.normal(sh, dtype, g, 2.0))
    ins = dict(y=val(npix, Cn), scale=(R.pow2((Cn,), g) if exact else R.normal((Cn,), F32, g)) if sc else None,
               shift=(R.ints((Cn,), g) * 0.25 if exact else R.normal((Cn,), F32, g)) if sc else None,
               dscale=(R.pow2((N,), g, -1, 1, signed=False) * torch.tensor([1.0, 0.0, 1.0]) if exact else R.normal((N,), F32, g).abs()) if ds else None,
               post=val(npix, Cn) if po else None)
    kw = lambda t: dict(scale=t['scale'], shift=t['shift'], dscale=t['dscale'])
    name = f'bnx_fwd-{"X" if exact else "T"}-{NAME[dtype]}-act{act}-form{sc}{ds}{po}'
    call = lambda S, t: S.bnx_fwd(t['y'], t['out'], hw, act, post=t['post'], **kw(t))
    ref = lambda f32=False: R.bnx_fwd(ins['y'], hw, act, ins['scale'], ins['shift'], ins['dscale'], ins['post'], f32=f32)
    if exact:
        out.append(Case(name, dtype, ins, dict(out=((npix, Cn), dtype, None)), call, refs=lambda: dict(out=ref()[0])))
    else:
        def check(tc):
            r, mag = ref()
            R.assert_transcendental(tc['out'], r, ref(True)[0].to(dtype), R.bound_e(r, mag, R.BNX_FWD_K, dtype), name, dtype)
        out.append(Case(name, dtype, ins, dict(out=((npix, Cn), dtype, None)), call, check=check))
    if dtype == F16 or (act == 1 and not sc) or po:
        return
    name = f'bnx_bwd-{"X" if exact else "T"}-{NAME[dtype]}-act{act}-form{sc}{ds}'
    insb = dict(ins, post=None, g=val(npix, Cn))
    callb = lambda S, t: S.bnx_bwd(t['g'], t['out'], hw, act, y=t['y'], **kw(t))
    refb = lambda f32=False: R.bnx_bwd(insb['g'], hw, act, insb['y'], insb['scale'], insb['shift'], insb['dscale'], f32=f32)
    if exact:
        out.append(Case(name, dtype, insb, dict(out=((npix, Cn), dtype, None)), callb, refs=lambda: dict(out=refb()[0])))
    else:
        def checkb(tc):
            r, mag = refb()
            R.assert_transcendental(tc['out'], r, refb(True)[0].to(dtype), R.bound_e(r, mag, R.BNX_BWD_K, dtype), name, dtype)
        out.append(Case(name, dtype, insb, dict(out=((npix, Cn), dtype, None)), callb, check=checkb))


def bnx_cases():
    out = []
    for dtype in ALL:
        for act in (0, 1):
            for form in ((1, 0, 0), (1, 1, 1), (0, 0, 0), (1, 1, 0), (0, 1, 1)):      # scale / dscale / post set or null
                _bnx_of(dtype, act, form, out)
    return out


def _dice_of(dtype, B, Cn, HW, CP, kind, out):
    g = R.gen(_seed('dice', dtype, B, Cn, HW, CP, kind))
    logits = R.normal((B, Cn, HW), F32, g, 3.0)
    target = (torch.rand(B, Cn, HW, generator=g) < 0.3).to(F32)
    if Cn > 1:
        target[:, -1] = 0       # an empty class: no Dice gradient there
    sums = R.dice_sums(logits, target)
    name = f'dice_bwd-T-{NAME[dtype]}-B{B}-C{Cn}-HW{HW}-CP{CP}-kind{kind}'

    def check(tc):
        ref, mag = R.dice_bwd(logits, target, sums, kind, 0.5)
        yard, _ = R.dice_bwd(logits, target, sums, kind, 0.5, f32=True)
        got = tc['out']
        R.assert_exact(got[..., Cn:], torch.zeros(B, HW, CP - Cn, dtype=torch.float64), name + ' padding')      # the padding channels are exactly zero
        R.assert_transcendental(got[..., :Cn], ref, yard.to(dtype), R.bound_e(ref, mag, R.DICE_BWD_K, dtype), name, dtype)
    out.append(Case(name, dtype, dict(logits=logits, target=target, sums=sums), dict(out=((B, HW, CP), dtype, None)),
                    lambda S, t: S.dice_bwd(t['logits'], t['target'], t['sums'], t['out'], loss_kind=kind, grad_scale=0.5), check=check))


def dice_cases():
    out = []
    for dtype in TRAIN:
        for B, Cn, HW, CP, kind in ((2, 1, 300, 8, 0), (2, 3, 77, 8, 0), (1, 3, 1, 16, 2), (3, 3, 260, 8, 1), (2, 1, 513, 16, 2)):
            _dice_of(dtype, B, Cn, HW, CP, kind, out)
    return out


def _gn_of(dtype, Cn, HW, out):
    G, N = 32, 2
    cpg = Cn // G
    H, W = (8, HW // 8)
    g = R.gen(_seed('gn', dtype, Cn, HW))
    S_ = min(max(HW // 1024, 1), 64)
    # forward, Rule X: every group holds mean +- dev in equal numbers (eps 0): rstd = 1 / dev, a power of two
    m = torch.randint(-2, 3, (N, 1, G), generator=g).to(torch.float64).repeat_interleave(cpg, 2)
    dev = torch.pow(2.0, torch.randint(-1, 2, (N, 1, G), generator=g).to(torch.float64)).repeat_interleave(cpg, 2)
    sign = ((torch.arange(HW).view(1, HW, 1) + torch.arange(Cn).view(1, 1, Cn)) % 2).to(torch.float64) * 2 - 1
    y = (m + dev * sign).to(dtype)
    gamma, beta = R.pow2((Cn,), g, -1, 1), R.ints((Cn,), g, -2, 2) * 0.5
    outs = dict(out=((N, H, W, Cn), dtype, None), part=((N, S_, Cn, 2), F32, None), ss=((N, Cn, 2), F32, None), stat=((N, G, 2), F32, None))

    def refs(y=y, gamma=gamma, beta=beta):
        ss, stat = R.gn_stats(y, gamma, beta, G, 0.0)
        return dict(ss=ss, stat=stat, out=R.gn_act(y, ss, H, W, 1)[0])
    out.append(Case(f'gn_forward-X-{NAME[dtype]}-C{Cn}-HW{HW}-up1', dtype, dict(y=y.view(N, H, W, Cn), gamma=gamma, beta=beta), outs,
                    lambda S, t: S.gn_forward(t['y'], t['gamma'], t['beta'], t['out'], t['part'], t['ss'], t['stat'], G, 1, 0.0), refs=refs))
    for up in (1, 2):       # rounded: statistics by Rule T (float32 yardstick), the activation from the kernel's own ss by Rule E
        yr, gr, br = R.normal((N, HW, Cn), dtype, g, 1.5), R.normal((Cn,), F32, g), R.normal((Cn,), F32, g)
        outs = dict(out=((N, H * up, W * up, Cn), dtype, None), part=((N, S_, Cn, 2), F32, None), ss=((N, Cn, 2), F32, None), stat=((N, G, 2), F32, None))
        name = f'gn_forward-T-{NAME[dtype]}-C{Cn}-HW{HW}-up{up}'

        def check(tc, yr=yr, gr=gr, br=br, up=up, name=name):
            ss, stat = R.gn_stats(yr, gr, br, G, 1e-5)
            with R.as_float32():
                ss32, stat32 = R.gn_stats(yr, gr, br, G, 1e-5)
            R.assert_transcendental(tc['stat'], stat, stat32, R.bound_e(stat, stat.abs(), 4, F32), name + ' stat', dtype)
            smag = torch.stack([ss[..., 0].abs(), d(br).abs().view(1, -1) + (ss[..., 1] - d(br).view(1, -1)).abs()], -1)
            R.assert_transcendental(tc['ss'], ss, ss32, R.bound_e(ss, smag, 7, F32), name + ' ss', dtype)

            def one():
                ref, mag = R.gn_act(yr, tc['ss'], H, W, up)
                R.assert_within(tc['out'], ref, R.bound_e(ref, mag, (1 if up == 1 else 1 + R.BILINEAR_K - 2) + 2, dtype), name + ' out')
            R.either_weights(one)
        out.append(Case(name, dtype, dict(y=yr.view(N, H, W, Cn), gamma=gr, beta=br), outs,
                        lambda S, t, up=up: S.gn_forward(t['y'], t['gamma'], t['beta'], t['out'], t['part'], t['ss'], t['stat'], G, up, 1e-5), check=check))
    if dtype == F16:
        return
    # backward, Rule X: dyadic values and teacher-forced dyadic statistics; HW x cpg is a power of two (the group means are exact)
    yb, gb = R.dyadic((N, HW, Cn), dtype, g, -4, 4, 0.5), R.dyadic((N, HW, Cn), dtype, g, -2, 2, 0.5)
    mean, rstd = R.ints((N, G), g, -1, 1), R.pow2((N, G), g, 0, 1, signed=False)
    gam, bet = R.pow2((Cn,), g, -1, 0), R.ints((Cn,), g, -2, 2) * 0.5
    scale = gam.view(1, Cn) * rstd.repeat_interleave(cpg, 1)
    ss = torch.stack([scale, bet.view(1, Cn) - mean.repeat_interleave(cpg, 1) * scale], -1)
    stat = torch.stack([mean, rstd], -1)
    dg0, db0 = R.ints((Cn,), g), R.ints((Cn,), g)

    def refs_b(yb=yb, gb=gb, gam=gam, ss=ss, stat=stat, dg0=dg0, db0=db0):
        r = R.gn_backward(yb, gb, gam, ss, stat, G)
        return dict(g=r['dy'], coef=r['coef'], dgamma=d(dg0) + r['dgamma'], dbeta=d(db0) + r['dbeta'])
    out.append(Case(f'gn_backward-X-{NAME[dtype]}-C{Cn}-HW{HW}', dtype, dict(y=yb, g=gb, gamma=gam, ss=ss, stat=stat),
                    dict(dgamma=((Cn,), F32, dg0), dbeta=((Cn,), F32, db0), part=((N, S_, Cn, 2), F32, None), coef=((N, G, 2), F32, None)),
                    lambda S, t: S.gn_backward(t['y'], t['g'], t['g'], t['gamma'], t['dgamma'], t['dbeta'], t['part'], t['ss'], t['stat'], t['coef'], G),
                    refs=refs_b))


def gn_cases():
    out = []
    for dtype in ALL:
        for Cn, HW in ((128, 64), (256, 64), (128, 2048)):      # one slab and two; vpc 16 / 32 (bf16), 32 / 64 (f32)
            _gn_of(dtype, Cn, HW, out)
    return out


def _sefc_of(dtype, act, Cn, Rn, out):
    N = 3
    exact = act == 0
    g = R.gen(_seed('sefc', dtype, act, Cn, Rn))
    val = (lambda *sh: R.dyadic(sh, dtype, g, -4, 4)) if exact else (lambda *sh: R.normal(sh, dtype, g))
    par = (lambda *sh: R.ints(sh, g, -2, 2) * 0.5) if exact else (lambda *sh: R.normal(sh, F32, g, 0.3))
    m, ds, w1, b1, w2, b2 = val(N, Cn), val(N, Cn), par(Rn, Cn), par(Rn), par(Cn, Rn), par(Cn)
    X = 'X' if exact else 'T'
    name = f'sefc_fwd-{X}-{NAME[dtype]}-act{act}-C{Cn}-R{Rn}'
    fw = lambda f32=False: R.sefc_fwd(m, w1, b1, w2, b2, act, f32=f32)
    call = lambda S, t: S.sefc_fwd(t['m'], t['s'], t['w1'], t['b1'], t['w2'], t['b2'], t['h'], act)
    ins, outs = dict(m=m, w1=w1, b1=b1, w2=w2, b2=b2), dict(s=((N, Cn), dtype, None), h=((N, Rn), F32, None))
    if exact:
        out.append(Case(name, dtype, ins, outs, call, refs=lambda: dict(s=fw()[0], h=fw()[1])))
    else:
        def check(tc):
            s_, h_, mag = fw()
            s32, h32, _ = fw(True)
            hmag = d(m).abs() @ d(w1).abs().t() + d(b1).abs()
            R.assert_within(tc['h'], h_, R.bound_r(h_, hmag, Cn + 1), name + ' h')
            R.assert_transcendental(tc['s'], s_, s32.to(dtype), R.bound_r(s_, mag, Rn + 1, dtype), name + ' s', dtype)
        out.append(Case(name, dtype, ins, outs, call, check=check))
    if dtype == F16:
        return
    h = (R.ints((N, Rn), g, -3, 3) * 0.5) if exact else R.normal((N, Rn), F32, g)
    zeros = lambda *sh: torch.zeros(*sh, dtype=F32)
    insb = dict(m=m, ds=ds, w1=w1, w2=w2, h=h)
    outsb = dict(dm=((N, Cn), dtype, None), dh=((N, Rn), F32, None), dw1=((Rn, Cn), F32, zeros(Rn, Cn)), db1=((Rn,), F32, zeros(Rn)),
                 dw2=((Cn, Rn), F32, zeros(Cn, Rn)), db2=((Cn,), F32, zeros(Cn)))
    bw = lambda f32=False: R.sefc_bwd(m, ds, w1, w2, h, act, f32=f32)
    callb = lambda S, t: S.sefc_bwd(t['m'], t['ds'], t['dm'], t['w1'], t['w2'], t['h'], t['dh'], act, t['dw1'], t['db1'], t['dw2'], t['db2'])
    name = f'sefc_bwd-{X}-{NAME[dtype]}-act{act}-C{Cn}-R{Rn}'
    if exact:
        out.append(Case(name, dtype, insb, outsb, callb, refs=lambda: {k: v for k, v in bw().items() if not k.endswith('_mag')}))
    else:
        def checkb(tc):
            r, r32 = bw(), bw(True)
            R.assert_transcendental(tc['dh'], r['dh'], r32['dh'], R.bound_r(r['dh'], r['dh_mag'], Cn + 8), name + ' dh', dtype)
            R.assert_transcendental(tc['dm'], r['dm'], r32['dm'].to(dtype), R.bound_r(r['dm'], r['dm_mag'], Rn + Cn + 8, dtype), name + ' dm', dtype)
            for k in ('dw1', 'db1', 'dw2', 'db2'):
                R.assert_transcendental(tc[k], r[k], r32[k], 64 * R.EPS32 * (r[k].abs() + r[k].abs().max()), f'{name} {k}', dtype)
        out.append(Case(name, dtype, insb, outsb, callb, check=checkb))


def sefc_cases():
    out = []
    for dtype in ALL:
        for act in (0, 1):
            for Cn, Rn in ((24, 6), (304, 19)):
                _sefc_of(dtype, act, Cn, Rn, out)
    return out


FAMILIES = dict(dwg=dwg_cases, bnx=bnx_cases, dice_bwd=dice_cases, groupnorm=gn_cases, sefc=sefc_cases, dw_and_seed=dw_cases, bn_finalize_train=bn_finalize_train_cases, bn_finalize_small=bn_finalize_small_cases, bn_finalize_eval=bn_finalize_eval_cases,
                bn_act=bn_act_cases, bn_bwd_reduce=bn_bwd_reduce_cases, bn_bwd_finalize=bn_bwd_finalize_cases, bn_bwd_apply=bn_bwd_apply_cases,
                bn_bwd_small=bn_bwd_small_cases, bn_bwd_chain=bn_bwd_chain_cases, plumbing=plumbing_cases, channel_sum=channel_sum_cases,
                tensor_stats=tensor_stats_cases, maxpool=maxpool_cases, bilinear=bilinear_cases, bin_mean=bin_mean_cases, image=image_cases,
                rearrange=rearrange_cases)

# a training-only sweep must refuse f16: (op, pointer count, integer arguments, float arguments) of one well-formed call each
TRAIN_ONLY = (('bn_finalize_small', 9, (4, 8), (0.1, 1e-5)), ('bn_bwd_small', 17, (4, 8, 0, 1, 0), ()), ('bn_bwd_reduce', 17, (4, 8, 0, 1, 0), ()),
              ('bn_bwd_finalize', 17, (4, 8, 0, 1, 0), ()), ('bn_bwd_apply', 17, (4, 8, 0, 1, 0), ()), ('masked_accum', 3, (32, 1), ()),
              ('pool2x2_accum', 2, (1, 2, 2, 8, 1), ()), ('channel_sum', 2, (4, 8, 8), ()), ('tensor_stats', 2, (4, 8, 1), ()),
              ('maxpool_bwd_idx', 3, (1, 2, 2, 8, 1), ()), ('bilinear_resize_adjoint', 2, (1, 2, 2, 4, 4, 8), ()), ('bilinear_adjoint', 2, (1, 2, 2, 8, 2), ()),
              ('bin_mean_bwd', 2, (1, 4, 4, 8, 2, 0), ()), ('se_dgate', 7, (1, 4, 8), ()), ('dw_wgrad', 3, (8, 0, 8, 0, 8, 0, 1, 4, 4, 8, 1), ()),
              ('cam_seed', 2, (1, 1, 4, 8), ()), ('dwg_bwd_data', 3, (1, 4, 4, 8, 4, 4, 3, 1, 1, 0), ()), ('dwg_bwd_w', 3, (1, 4, 4, 8, 4, 4, 3, 1, 1), ()),
              ('bnx_bwd', 6, (4, 4, 8, 0), ()), ('dice_bwd', 4, (1, 1, 4, 8, 0), (1.0,)), ('gn_backward', 10, (1, 4, 32, 4), ()),
              ('sefc_bwd', 11, (1, 8, 2, 0), ()))
