"""The cases the CPU and the GPU tests of the logit histograms share (tests/test_curves.py, tests/test_gpu_curves.py), their inputs and reference.

Every case is built so that ALL pixels compare between the kernel's f32 rule and the float64 reference, with no exclusion share.  Drawn logits
(N(0, 3^2)) go through ``sanitize``: a value whose float64 ``p * 256`` lies within MARGIN = 1e-3 of an integer, or whose ``p`` is below 2^-20 or
above 1 - 2^-20, is replaced by MID, the float32 logit of the middle of bin 37; the two exact values +-0 (p = 0.5 on any arithmetic) are exempt.
An f32 sigmoid is within 2^-22 relative of the float64 one (expf 1 ulp plus two roundings), so ``p * 256`` moves by less than 256 * 2^-22 = 6.1e-5,
a sixteenth of the margin.  The saturated cases hold +-30 on purpose (the kernel's ballot path alone): there ``p * 256`` is within 2.4e-11 of 0 or
of 256 and the CLAMP decides -- p = 0 or a tiny p give bin 0, p = 1 or 1 - tiny give bin 255 under any rounding -- so they are outside the margin
rule by construction, and tests/test_curves.py pins that both rules give exactly those bins.

Targets are 0 in about 70 % of the pixels and otherwise one of 1, 0.5, -3, 255: positive is ``!= 0``, not ``== 1``."""
import functools
from collections import namedtuple

import numpy as np

import curves_ref as R

MARGIN = 1e-3
EDGE = 2.0 ** -20
MID = np.float32(np.log(37.5 / 256 / (1 - 37.5 / 256)))
SATURATED = np.float32(30.0)

Case = namedtuple('Case', 'id shape kind seed')

CASES = [
    Case('odd-2x3x37x53', (2, 3, 37, 53), 'drawn', 11),          # H * W = 1961: plane bases off the 16-byte grid, scalar head and tail
    Case('pixel-1x1x1x1', (1, 1, 1, 1), 'drawn', 12),
    Case('aligned-1x2x64x64', (1, 2, 64, 64), 'drawn', 13),
    Case('split-3x1x130x200', (3, 1, 130, 200), 'drawn', 14),    # 26000 pixels per plane: several workgroups, the global atomics merge
    Case('saturated-t0', (2, 2, 19, 23), 'sat-zeros', 15),       # every logit +-30: the hot cells only
    Case('saturated-t1', (2, 2, 19, 23), 'sat-ones', 16),
    Case('saturated-checker', (1, 1, 96, 100), 'sat-checker', 17),
    Case('one-bin', (1, 2, 45, 47), 'constant', 18),             # every logit MID: one LDS address per label
    Case('zeros-row', (1, 1, 2, 50), 'zeros', 19),               # 0.0, -0.0, ...: the threshold itself, p = 0.5 exactly, bin 127, not set
]
IDS = [c.id for c in CASES]


def margin_ok(z):
    """Per value: +-0, or float64 p * 256 at least MARGIN from every integer and p inside [2^-20, 1 - 2^-20]."""
    z = np.asarray(z)
    p = R.sigmoid64(z)
    s = p * 256.0
    return (z == 0) | ((np.abs(s - np.rint(s)) >= MARGIN) & (p >= EDGE) & (p <= 1.0 - EDGE))


def sanitize(z):
    z = np.array(z, dtype=np.float32)
    z[~margin_ok(z)] = MID
    return z


def draw_logits(rng, shape, sigma=3.0):
    return sanitize((rng.standard_normal(shape) * sigma).astype(np.float32))


def draw_target(rng, shape):
    t = rng.choice(np.array([1.0, 0.5, -3.0, 255.0], np.float32), size=shape)
    t[rng.random(shape) < 0.7] = 0.0
    return t.astype(np.float32)


def checkerboard(shape):
    return ((np.indices(shape[2:]).sum(axis=0) % 2) * np.ones(shape)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(logits, target): float32 NCHW, read-only."""
    rng = np.random.default_rng(case.seed)
    if case.kind == 'drawn':
        z, t = draw_logits(rng, case.shape), draw_target(rng, case.shape)
    elif case.kind.startswith('sat-'):
        z = np.where(rng.random(case.shape) < 0.5, SATURATED, -SATURATED).astype(np.float32)
        t = {'sat-zeros': np.zeros(case.shape, np.float32), 'sat-ones': np.ones(case.shape, np.float32),
             'sat-checker': checkerboard(case.shape)}[case.kind]
    elif case.kind == 'constant':
        z, t = np.full(case.shape, MID, np.float32), draw_target(rng, case.shape)
    elif case.kind == 'zeros':
        z = np.where(np.arange(case.shape[3]) % 2 == 0, np.float32(0.0), np.float32(-0.0)) * np.ones(case.shape, np.float32)
        z = z.astype(np.float32)
        t = checkerboard(case.shape)
    else:
        raise ValueError(case.kind)
    z.setflags(write=False)
    t.setflags(write=False)
    return z, t


@functools.lru_cache(maxsize=None)
def reference(case):
    """tests/curves_ref.py on the case, computed once and shared; read-only."""
    z, t = inputs(case)
    h = R.histogram(z, t)
    h.setflags(write=False)
    return h
