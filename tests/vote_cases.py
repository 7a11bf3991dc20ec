"""The cases the CPU and the GPU tests of the voted epilogue share (tests/test_vote.py, tests/test_gpu_vote.py), their logits and their reference.

Logits are seeded N(0, 3) draws, every |z| < 0.01 pushed to +-0.01 so that ``z > 0`` decides a member's vote on any arithmetic.  Members are
independent draws, so a wrong un-view changes the result.  Member m has 1 + m % 2 classes and votes with channel (m // 2) % classes."""
import functools
from collections import namedtuple

import numpy as np

import vote_ref as R

Case = namedtuple('Case', 'id H W oh ow N views mode tables seed')

# (H, W) -> (out_h, out_w), then (N, view code of every member) twice per shape: M in {1, 2, 3, 5, 8}, even M so that majority ties occur
_SHAPES = [
    ((1, 1), (1, 1), [(1, (0,)), (3, (0, 0))]),
    ((5, 7), (5, 7), [(3, (1, 2, 3)), (1, (0, 1, 2, 3, 0))]),
    ((32, 32), (37, 37), [(1, (0, 1, 2, 3, 4, 5, 6, 7)), (3, (5, 6))]),
    ((64, 64), (23, 50), [(3, (7, 6, 5, 4, 3, 2, 1, 0)), (1, (4, 1, 7, 2, 5))]),
    ((33, 33), (96, 96), [(1, (0, 1, 2, 3, 4, 5, 6, 7)), (3, (6, 3, 5))]),
    ((64, 96), (100, 64), [(3, (2, 1)), (1, (3, 0, 1, 2, 3))]),
    ((40, 40), (300, 300), [(3, (4, 0)), (1, (7,))]),          # 19 x 3 workgroups per frame, the last with 5 of its 8 tiles past the frame
]


# seeds are 1000 + the case's index, except where that draw has a soft near-tie (|pbar64 - 0.5| <= (M + 4) 2^-23 at some pixel; seed 1024 draws two
# nearly opposite logits at one pixel of this case, pbar64 = 0.50000048): tests/test_vote.py pins that no case has one, so that the GPU tests compare every pixel
_RESEED = {'40x40-300x300-N3-M2-soft-null': 2024}


def _cases():
    out = []
    for (H, W), (oh, ow), members in _SHAPES:
        for k, (N, views) in enumerate(members):
            for mode in (0, 1):
                tables = bool((k + mode) % 2)             # cv2_nearest_index tables and null tables, both with every shape and mode
                cid = f'{H}x{W}-{oh}x{ow}-N{N}-M{len(views)}-{"majority" if mode else "soft"}-{"cv2" if tables else "null"}'
                out.append(Case(cid, H, W, oh, ow, N, views, mode, tables, _RESEED.get(cid, 1000 + len(out))))
    return out


CASES = _cases()
IDS = [c.id for c in CASES]


def member_layout(case):
    """(classes, channel) of every member."""
    classes = [1 + m % 2 for m in range(len(case.views))]
    return classes, [(m // 2) % c for m, c in enumerate(classes)]


def draw_logits(rng, shape):
    z = (rng.standard_normal(shape) * 3.0).astype(np.float32)
    small = np.abs(z) < 0.01
    z[small] = np.where(z[small] >= 0, np.float32(0.01), np.float32(-0.01))
    return z


@functools.lru_cache(maxsize=None)
def inputs(case):
    """(members, classes, channels, rows, cols): float32 logits in every member's view coordinates, index tables (None = the centre rule)."""
    from oct_segmentation_amd.predict import cv2_nearest_index
    rng = np.random.default_rng(case.seed)
    classes, channels = member_layout(case)
    members = []
    for v, c in zip(case.views, classes):
        hm, wm = (case.W, case.H) if v & 4 else (case.H, case.W)
        z = draw_logits(rng, (case.N, c, hm, wm))
        z.setflags(write=False)
        members.append(z)
    rows = cv2_nearest_index(case.H, case.oh) if case.tables else None
    cols = cv2_nearest_index(case.W, case.ow) if case.tables else None
    return tuple(members), classes, channels, rows, cols


@functools.lru_cache(maxsize=None)
def reference(case):
    """tests/vote_ref.py on the case, computed once and shared; the arrays are read-only."""
    members, _, channels, rows, cols = inputs(case)
    ref = R.vote(members, channels, case.views, (case.oh, case.ow), rows, cols, case.mode)
    for a in ref.values():
        a.setflags(write=False)
    return ref


def prob_bound(M):
    """|prob - pbar64| on the GPU: one sigmoid is within 2^-22 relative (expf 1 ulp plus two roundings), a sequential f32 sum of M terms in [0, 1]
    divided by M adds at most M * 2^-24; the bound doubles that."""
    return (M + 4) * 2.0 ** -23
