"""Slice interpolation without a GPU: the ABI and its refusals, the wrappers' refusals, gap_plan on hand-written presence tables, the properties
and known answers of the scipy restatement (tests/interp_ref.py), and the gaps of the golden excerpt."""
import ctypes as C
import functools
import json
import os
import re

import numpy as np
import pytest
import torch

import interp_ref as R
from analysis_ref import load_fixture
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import interp

FIXTURE = os.path.join(os.path.dirname(__file__), 'golden', 'pullback_demo_excerpt.npz')


# ---- 1. ABI
def test_symbols_of_the_interpolation_entry_points():
    i, p, z = C.c_int, C.c_void_p, C.c_size_t
    want = {
        'octseg_signed_distance_scratch_bytes': (z, [i, i, i, i]),
        'octseg_stack_signed_distance': (i, [p, i, i, i, i, p, z, p, p]),
        'octseg_signed_blend': (i, [p, i, i, i, i, p, i, p, i, p, p]),
    }
    for name, sig in want.items():
        assert L.SYMBOLS[name] == sig, name
        assert hasattr(L.lib(), name)
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'octseg.h')).read()
    flat = re.sub(r'\s+', ' ', re.sub(r'/\*.*?\*/', ' ', header, flags=re.S))
    for decl in ('size_t octseg_signed_distance_scratch_bytes(int N, int H, int W, int channels);',
                 'int octseg_stack_signed_distance(const float* stack, int N, int H, int W, int channels, void* scratch, size_t scratch_bytes, '
                 'int* sd2, void* stream);',
                 'int octseg_signed_blend(const int* sd2, int K, int H, int W, int channels, const int* plan, int M, float* out, int N_out, '
                 'int* made, void* stream);'):
        assert decl in flat.replace(' ,', ','), decl
    assert interp.DIST_NONE == 0x7fffffff == R.NONE and interp.MAX_WEIGHT == 32767 == R.MAX_WEIGHT


def test_scratch_formula():
    """Two sets of bit planes, two uint16 column maps (4 bytes per pixel and channel), two int32 flags per plane; every array on a 256-byte
    boundary."""
    lib = L.lib()
    al = lambda v: (v + 255) // 256 * 256
    for n, h, w, c in ((1, 1, 1, 1), (2, 33, 65, 4), (3, 97, 130, 5), (1, 750, 750, 4), (7, 64, 64, 16)):
        planes, words = n * c, h * ((w + 63) // 64)
        want = 2 * al(planes * words * 8) + 2 * al(planes * h * w * 2) + al(2 * planes * 4)
        assert lib.octseg_signed_distance_scratch_bytes(n, h, w, c) == want, (n, h, w, c)
    for bad in ((0, 8, 8, 1), (1, 0, 8, 1), (1, 8, 0, 1), (1, 4097, 8, 1), (1, 8, 4097, 1), (1, 8, 8, 0), (1, 8, 8, 17), (-1, 8, 8, 1)):
        assert lib.octseg_signed_distance_scratch_bytes(*bad) == 0, bad


def test_library_refuses_before_any_launch():
    lib = L.lib()
    buf = (C.c_char * 4096)()                                # host buffers: the calls below must return before they touch a pointer
    other = (C.c_char * 64)()
    a, b = C.cast(buf, C.c_void_p), C.cast(other, C.c_void_p)
    odd = C.c_void_p(a.value + 4)
    big = 1 << 40
    BAD_SHAPE, BAD_ARG = -1, -5
    sd = lib.octseg_stack_signed_distance
    assert sd(None, 1, 8, 8, 1, a, big, b, None) == BAD_ARG
    assert sd(a, 1, 8, 8, 1, None, big, b, None) == BAD_ARG
    assert sd(a, 1, 8, 8, 1, a, big, None, None) == BAD_ARG
    assert sd(a, 1, 8, 8, 1, odd, big, b, None) == BAD_ARG and b'aligned' in lib.octseg_last_error()
    assert sd(a, 1, 8, 8, 1, a, 16, b, None) == BAD_ARG and b'scratch is smaller' in lib.octseg_last_error()
    assert sd(a, 1, 8, 8, 1, a, lib.octseg_signed_distance_scratch_bytes(1, 8, 8, 1) - 1, b, None) == BAD_ARG
    assert sd(a, 1, 8, 8, 1, b, big, a, None) == BAD_ARG and b'alias' in lib.octseg_last_error()
    for n, h, w, c in ((0, 8, 8, 1), (1, 0, 8, 1), (1, 8, -1, 1), (1, 4097, 8, 1), (1, 8, 4097, 1), (1, 8, 8, 0), (1, 8, 8, 17)):
        assert sd(a, n, h, w, c, a, big, b, None) == BAD_SHAPE, (n, h, w, c)
    bl = lib.octseg_signed_blend
    assert bl(None, 1, 8, 8, 1, a, 1, b, 1, None, None) == BAD_ARG
    assert bl(a, 1, 8, 8, 1, None, 1, b, 1, None, None) == BAD_ARG
    assert bl(a, 1, 8, 8, 1, a, 1, None, 1, None, None) == BAD_ARG
    assert bl(a, 1, 8, 8, 1, b, 1, a, 1, None, None) == BAD_ARG and b'alias' in lib.octseg_last_error()
    for k, h, w, c, m, n_out in ((0, 8, 8, 1, 1, 1), (1, 0, 8, 1, 1, 1), (1, 8, 0, 1, 1, 1), (1, 4097, 8, 1, 1, 1), (1, 8, 4097, 1, 1, 1),
                                 (1, 8, 8, 0, 1, 1), (1, 8, 8, 17, 1, 1), (1, 8, 8, 1, 0, 1), (1, 8, 8, 1, -3, 1), (1, 8, 8, 1, 1, 0)):
        assert bl(a, k, h, w, c, a, m, b, n_out, None, None) == BAD_SHAPE, (k, h, w, c, m, n_out)
    assert not any(buf.raw) and not any(other.raw)


# ---- 2. the wrappers' refusals
def test_wrappers_refuse_host_tensors_and_bad_plans():
    cpu = torch.zeros((2, 4, 4, 3))
    for bad in (cpu, cpu.numpy(), cpu.double(), cpu[0]):
        for fn in (interp.signed_distance_stack, interp.bridge_gaps, lambda s: interp.resample_stack(s, 2)):
            with pytest.raises(ValueError, match='float32 CUDA tensor'):
                fn(bad)
    with pytest.raises(ValueError, match='sd2 must be'):
        interp.blend_planes(torch.zeros((2, 3, 4, 4), dtype=torch.int32), [[0, 0, 0, 1, 1, 1]], cpu)
    for factor in (0, -1, 1.5, True, 32768):
        with pytest.raises(ValueError, match='factor'):
            interp.resample_stack(cpu, factor)
    ok = [[0, 0, 0, 1, 1, 1], [1, 0, 0, 1, 1, 2], [0, 1, 1, 1, 0, 32767]]
    assert interp.check_plan(ok, 2, 3, 2).dtype == np.int32 and interp.check_plan(torch.tensor(ok), 2, 3, 2).tolist() == ok
    cases = {'same output plane': ok + [[0, 0, 1, 1, 1, 0]], 'both weights 0': [[0, 0, 0, 1, 0, 0]], 'weights': [[0, 0, 0, 1, 32768, 1]],
             'weights ': [[0, 0, 0, 1, 1, -1]], 'channel': [[3, 0, 0, 1, 1, 1]], 'channel ': [[-1, 0, 0, 1, 1, 1]], 'output slice': [[0, 2, 0, 1, 1, 1]],
             'output slice ': [[0, -1, 0, 1, 1, 1]], 'key slice': [[0, 0, 2, 1, 1, 1]], 'key slice ': [[0, 0, 0, -1, 1, 1]], 'M >= 1': [],
             'M >= 1 ': [[0, 0, 0, 1, 1]], 'M >= 1  ': [[0.0, 0, 0, 1, 1, 1]]}
    for match, plan in cases.items():
        with pytest.raises(ValueError, match=match.strip()):
            interp.check_plan(plan, 2, 3, 2)


# ---- 3. gap_plan on hand-written presence tables
def table(n, **runs):
    """present [n, len(runs)]: every channel from a string of n characters, '#' present and '.' absent."""
    cols = [np.array([ch == '#' for ch in s]) for s in runs.values()]
    assert all(c.size == n for c in cols)
    return np.stack(cols, axis=1)


def both(present, max_gap, frames=None):
    got = interp.gap_plan(present, max_gap, frames)
    assert got.dtype == np.int32 and got.ndim == 2 and got.shape[1] == 6
    assert np.array_equal(got, R.gap_plan(present, max_gap, frames))
    return got.tolist()


def test_gap_plan_gaps_of_one_two_and_three():
    #                     0123456789012
    p = table(13, a='##.##..##...#')
    one = [[0, 2, 1, 3, 1, 1]]
    two = [[0, 5, 4, 7, 2, 1], [0, 6, 4, 7, 1, 2]]
    three = [[0, 9, 8, 12, 3, 1], [0, 10, 8, 12, 2, 2], [0, 11, 8, 12, 1, 3]]
    assert both(p, 0) == []
    assert both(p, 1) == one
    assert both(p, 2) == one + two
    assert both(p, 3) == one + two + three
    assert both(p, 50) == one + two + three


def test_gap_plan_never_extrapolates_and_skips_absent_and_full_channels():
    p = table(6, ends='..##..', never='......', always='######', one='...#..', inner='.#.#..')
    for g in (1, 2, 6):
        assert both(p, g) == [[4, 2, 1, 3, 1, 1]]            # the runs that touch an end, the absent and the full channel give nothing


def test_gap_plan_rejected_frames():
    p = table(7, a='#######', b='##...##', c='.......')
    mid = both(p, 1, frames=[3])
    # every channel is re-made at slice 3, whatever its neighbours hold; b's own gap of three stays unfilled at max_gap=1
    assert mid == [[0, 3, 2, 4, 1, 1], [1, 3, 2, 4, 1, 1], [2, 3, 2, 4, 1, 1]]
    run = both(p, 2, frames=[3, 4])
    assert run == [[c, k, 2, 5, 5 - k, k - 2] for c in range(3) for k in (3, 4)]
    first = both(p, 1, frames=[0])
    assert first == [[c, 0, 1, 1, 1, 0] for c in range(3)]   # a copy of the nearest accepted slice: weight 0 on the missing side
    last = both(p, 2, frames=[5, 6])
    assert last == [[c, k, 4, 4, 1, 0] for c in range(3) for k in (5, 6)]
    # b's gap with max_gap=3: the rejected slice 3 keeps the rows of the frames rule, 2 and 4 are made from b's present slices 1 and 5
    mixed = both(p, 3, frames=[3])
    assert [r for r in mixed if r[0] == 1] == [[1, 2, 1, 5, 3, 1], [1, 3, 2, 4, 1, 1], [1, 4, 1, 5, 1, 3]]
    # a rejected slice is never a neighbour: a's slices stay, its rejected one is made from 2 and 4
    assert [r for r in mixed if r[0] == 0] == [[0, 3, 2, 4, 1, 1]]
    for frames, g in (([3, 4], 1), ([0, 1, 2], 2), ([6], 0), (list(range(7)), 7)):
        with pytest.raises(ValueError):
            interp.gap_plan(p, g, frames)
        with pytest.raises(ValueError):
            R.gap_plan(p, g, frames)
    for frames in ([7], [-1], [1.5], [True]):
        with pytest.raises(ValueError, match='frames'):
            interp.gap_plan(p, 1, frames)
    with pytest.raises(ValueError, match='max_gap'):
        interp.gap_plan(p, -1)
    with pytest.raises(ValueError, match='present'):
        interp.gap_plan(p.astype(np.int32), 1)


def test_resample_plan_rows():
    assert interp.resample_plan(0, 1, 3, 2).tolist() == [[0, 0, 0, 0, 1, 0], [1, 0, 0, 0, 1, 0], [0, 1, 0, 1, 2, 1], [1, 1, 0, 1, 2, 1],
                                                         [0, 2, 0, 1, 1, 2], [1, 2, 0, 1, 1, 2], [0, 3, 1, 1, 1, 0], [1, 3, 1, 1, 1, 0]]
    # a later window: key numbers count from its first slice, whose own plane the window before it wrote
    assert interp.resample_plan(2, 3, 2, 1, with_first=False).tolist() == [[0, 5, 0, 1, 1, 1], [0, 6, 1, 1, 1, 0]]
    assert interp.resample_plan(0, 2, 1, 1).tolist() == [[0, 0, 0, 0, 1, 0], [0, 1, 1, 1, 1, 0], [0, 2, 2, 2, 1, 0]]


def test_bridge_report_is_json_clean():
    plan = np.array([[3, 14, 13, 15, 1, 1], [0, 2, 1, 4, 2, 1], [0, 3, 1, 4, 1, 2]], np.int32)
    names = [f'f{i:02d}' for i in range(20)]
    rep = interp.bridge_report(plan, np.array([5, 7, 9], np.int32), names)
    assert list(rep) == ['Lumen', 'Fibrous cap', 'Lipid core', 'Vasa vasorum']
    assert rep['Lumen'] == {'slice': [2, 3], 'lo': [1, 1], 'hi': [4, 4], 'w_lo': [2, 1], 'w_hi': [1, 2], 'pixels': [7, 9], 'image': ['f02', 'f03']}
    assert rep['Vasa vasorum']['slice'] == [14] and rep['Vasa vasorum']['pixels'] == [5] and rep['Fibrous cap']['slice'] == []
    assert json.loads(json.dumps(rep)) == rep
    assert interp.bridge_report(plan[:0], [], None)['Lumen']['slice'] == []
    assert interp.bridge_report(plan[1:], [7, 9], None, classes=['x'])['x']['image'] == [None, None]
    with pytest.raises(ValueError):
        interp.bridge_report(plan, [1, 2], names)


# ---- 4. properties of the reference blend
@functools.lru_cache(maxsize=None)
def planes():
    rng = np.random.RandomState(5)
    small, large = R.disc(30, 30, 9), R.disc(32, 33, 21)
    assert (small & ~large).sum() == 0
    blobs = rng.rand(64, 64) < 0.5
    out = {'small': small, 'large': large, 'blobs': blobs, 'sparse': rng.rand(64, 64) < 0.02, 'empty': np.zeros((64, 64), bool),
           'full': np.ones((64, 64), bool), 'left': np.mgrid[:64, :64][1] < 32}
    out['right'] = ~out['left']
    return {k: (m, R.sd2_plane(m)) for k, m in out.items()}


WEIGHTS = [(1, 1), (1, 2), (3, 1), (32767, 1), (1, 32767), (32767, 32767), (7, 5)]


def test_sd2_of_the_reference_is_never_zero_and_signed_by_the_mask():
    for name, (m, s) in planes().items():
        assert (s != 0).all() and np.array_equal(s > 0, m), name
    assert (planes()['empty'][1] == -R.NONE).all() and (planes()['full'][1] == R.NONE).all()
    m, s = planes()['small']
    # radius 9 about (30, 30): the nearest clear pixels of the centre are (29 | 31, 39), 1 + 81 away -- (30, 40) is 100 away
    assert s[30, 30] == 82 and s[30, 40] == -1 and s[30, 39] == 1 and s[31, 39] == -1


def test_blend_of_a_plane_with_itself_and_zero_weights():
    for name, (m, s) in planes().items():
        for wa, wb in WEIGHTS:
            assert np.array_equal(R.blend(s, s, wa, wb), m), name
        for other, (_, t) in planes().items():
            assert np.array_equal(R.blend(s, t, 5, 0), m) and np.array_equal(R.blend(t, s, 0, 1), m)


def test_blend_is_symmetric_under_swapping_sides_with_their_weights():
    names = sorted(planes())
    for a in names:
        for b in names:
            for wa, wb in WEIGHTS:
                assert np.array_equal(R.blend(planes()[a][1], planes()[b][1], wa, wb), R.blend(planes()[b][1], planes()[a][1], wb, wa)), (a, b)


def test_blend_of_nested_planes_stays_between_them():
    nested = [('small', 'large'), ('empty', 'blobs'), ('blobs', 'full'), ('empty', 'full'), ('small', 'full'), ('empty', 'small')]
    for a, b in nested:
        (ma, sa), (mb, sb) = planes()[a], planes()[b]
        assert not (ma & ~mb).any()
        for wa, wb in WEIGHTS:
            got = R.blend(sa, sb, wa, wb)
            assert not (ma & ~got).any() and not (got & ~mb).any(), (a, b, wa, wb)


def test_blend_of_empty_against_full_follows_the_larger_weight():
    e, f = planes()['empty'][1], planes()['full'][1]
    assert not R.blend(e, f, 1, 1).any() and not R.blend(f, e, 32767, 32767).any()        # the tie is clear
    assert R.blend(e, f, 1, 2).all() and R.blend(f, e, 3, 1).all()
    assert not R.blend(e, f, 2, 1).any() and not R.blend(f, e, 1, 32767).any()
    # an infinite side beats a finite one whatever the weights
    d = planes()['blobs']
    assert not R.blend(e, d[1], 1, 32767).any() and R.blend(f, d[1], 1, 32767).all()


def test_blend_of_complementary_half_planes_is_empty_at_equal_weights():
    l, r = planes()['left'][1], planes()['right'][1]
    assert not R.blend(l, r, 1, 1).any() and not R.blend(r, l, 4, 4).any()               # +k^2 against -k^2 everywhere: the tie rule
    assert np.array_equal(R.blend(l, r, 2, 1), planes()['left'][0]) and np.array_equal(R.blend(l, r, 1, 2), planes()['right'][0])


# ---- 5. known answers, measured with scipy
def test_known_answers_of_discs():
    a, b = R.sd2_plane(R.disc(32, 32, 10)), R.sd2_plane(R.disc(32, 32, 20))
    assert int(R.blend(a, b, 1, 1).sum()) == 709                     # radius about 15.0
    assert int(R.blend(a, b, 3, 1).sum()) == 473 and int(R.blend(a, b, 1, 3).sum()) == 997
    # no correspondence between slices: discs that do not overlap vanish
    assert int(R.blend(R.sd2_plane(R.disc(32, 20, 8)), R.sd2_plane(R.disc(32, 40, 8)), 1, 1).sum()) == 0
    m = R.blend(R.sd2_plane(R.disc(32, 24, 8)), R.sd2_plane(R.disc(32, 34, 8)), 1, 1)
    assert int(m.sum()) == 145 and np.nonzero(m)[1].mean() == 29.0


# ---- 6. the golden excerpt
@functools.lru_cache(maxsize=None)
def golden():
    st = load_fixture(FIXTURE)['stack']
    assert st.shape == (48, 750, 750, 4)
    return st, (st != 0).any(axis=(1, 2))


def present_pairs(col):
    idx = np.flatnonzero(col)
    return [(int(a), int(b)) for a, b in zip(idx[:-1], idx[1:]) if b - a > 1]


def test_golden_excerpt_presence_and_gaps():
    st, present = golden()
    assert present[:, 0].all()
    assert present_pairs(present[:, 1]) == present_pairs(present[:, 2]) == [(1, 8), (8, 12), (13, 28), (30, 46)]
    want2 = [[3, 14, 13, 15, 1, 1], [3, 25, 24, 26, 1, 1], [3, 36, 35, 38, 2, 1], [3, 37, 35, 38, 1, 2]]
    assert both(present, 1) == want2[:2] and both(present, 2) == want2
    plan3 = both(present, 3)
    for c in (1, 2):
        assert [r for r in plan3 if r[0] == c] == [[c, 9, 8, 12, 3, 1], [c, 10, 8, 12, 2, 2], [c, 11, 8, 12, 1, 3]]
    assert not [r for r in plan3 if r[0] == 0]
    out, plan, made = R.bridge(st, 2)
    assert plan.tolist() == want2 and made.tolist() == [0, 0, 3, 0]
    named = {(o, c) for c, o, *_ in want2}
    for o in range(48):
        for c in range(4):
            if (o, c) not in named:
                assert np.array_equal(out[o, :, :, c], st[o, :, :, c])
    assert interp.bridge_report(plan, made, [f'frame_{i}' for i in range(48)])['Vasa vasorum']['pixels'] == [0, 0, 3, 0]


def test_golden_excerpt_drop_and_restore_of_lumen_slices():
    """The floor is a sanity bound on the METHOD (the reference alone reaches 0.981 .. 0.990), not on the kernel."""
    st, _ = golden()
    sd2 = R.sd2_stack(st[0:8, :, :, :1])
    for k in range(1, 7):
        assert R.dice(R.blend(sd2[k - 1, 0], sd2[k + 1, 0], 1, 1), st[k, :, :, 0]) >= 0.95, k
