"""Host half of the polar plaque profile (oct_segmentation_amd/polar.py) on hand-built profiles, the argument checks of the two ABI calls and
of the Python wrappers.  No GPU: the refusals happen before any launch."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import polar_ref as P
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import polar
from oct_segmentation_amd.postprocess import CLASS_COLORS_RGB

IN, OUT, LAST, HITS, RUNS = range(5)


def _prof(n=1, sc=4):
    return np.zeros((n, sc, 360, 5), np.int32)


def _put(prof, n, c, degrees, first, out, last=None):
    """One run first..out on the given degrees (and, with `last`, a second single step there)."""
    for a in degrees:
        a %= 360
        two = last is not None and last > out
        prof[n, c, a] = (first, out, last if two else out, out - first + 1 + (1 if two else 0), 2 if two else 1)


def _check_against_ref(prof):
    s = polar.summarize(prof)
    for n in range(prof.shape[0]):
        for c in range(prof.shape[1]):
            want = P.summary(prof[n, c])
            got = {k: s[k][n, c] for k in want}
            assert got == want, (n, c, got, want)
    return s


def test_summarize_none_and_all_met():
    prof = _prof(2)
    _put(prof, 1, 0, range(360), 3, 9)
    s = _check_against_ref(prof)
    assert (s['arc'][0] == 0).all() and (s['arc_max'][0] == 0).all() and (s['arc_start'][0] == -1).all()
    assert (s['thick_min'][0] == 0).all() and (s['thick_median'][0] == 0).all() and (s['depth_min'][0] == 0).all()
    assert (s['arc'][1, 0], s['arc_max'][1, 0], s['arc_start'][1, 0]) == (360, 360, 0)
    assert (s['thick_min'][1, 0], s['thick_max'][1, 0], s['thick_median'][1, 0], s['depth_min'][1, 0]) == (7, 7, 7.0, 3)
    assert s['thick_median'].dtype == np.float64


def test_summarize_wrapping_run_and_ties():
    prof = _prof(3)
    _put(prof, 0, 1, range(350, 371), 5, 6)                    # 350 .. 359, 0 .. 10: one run of 21 through 0
    _put(prof, 0, 1, range(100, 110), 2, 9)                    # and a shorter one
    _put(prof, 1, 2, range(200, 230), 4, 4)                    # two equal runs: the smaller start wins
    _put(prof, 1, 2, range(20, 50), 4, 4)
    _put(prof, 2, 0, list(range(340, 360)) + list(range(0, 5)), 1, 1)   # a wrapping run of 25 against a later plain one of 25
    _put(prof, 2, 0, range(100, 125), 1, 1)
    _put(prof, 2, 3, [359], 7, 8)                              # a single degree at the end of the circle
    s = _check_against_ref(prof)
    assert (s['arc'][0, 1], s['arc_max'][0, 1], s['arc_start'][0, 1]) == (31, 21, 350)
    assert (s['thick_min'][0, 1], s['thick_max'][0, 1], s['depth_min'][0, 1]) == (2, 8, 2)
    assert (s['arc'][1, 2], s['arc_max'][1, 2], s['arc_start'][1, 2]) == (60, 30, 20)
    assert (s['arc'][2, 0], s['arc_max'][2, 0], s['arc_start'][2, 0]) == (50, 25, 100)
    assert (s['arc'][2, 3], s['arc_max'][2, 3], s['arc_start'][2, 3]) == (1, 1, 359)


def test_summarize_median_of_even_and_odd_counts():
    prof = _prof(2, 1)
    for a, (f, o) in enumerate([(1, 1), (1, 4), (2, 11)]):     # thicknesses 1, 4, 10: odd count
        _put(prof, 0, 0, [a], f, o)
    for a, (f, o) in enumerate([(1, 1), (1, 4), (2, 11), (5, 9)]):   # 1, 4, 10, 5: even count, median 4.5
        _put(prof, 1, 0, [a], f, o)
    s = _check_against_ref(prof)
    assert s['thick_median'][0, 0] == 4.0 and s['thick_median'][1, 0] == 4.5
    assert s['depth_min'][0, 0] == 1 and s['thick_max'][1, 0] == 10


def _cap_lipid():
    """Slice 0: cap 4..(4 + t - 1) on 300 .. 59 with lipid behind it on 350 .. 39; slice 1: lipid in FRONT of the cap; slice 2: nothing."""
    prof = _prof(3)
    for a in range(300, 420):
        t = 9 if a % 360 in (355, 20, 30) else 12 + (a % 7)    # the minimum 9 is attained at 20, 30 and 355: argmin 20
        _put(prof, 0, 1, [a], 4, 4 + t - 1)
    _put(prof, 0, 2, range(350, 400), 40, 60)
    _put(prof, 0, 2, [100], 40, 60)                            # lipid where no cap is: no overlap
    _put(prof, 1, 1, range(0, 90), 50, 60)
    _put(prof, 1, 2, range(0, 90), 10, 20)
    return prof


def test_overlap_and_argmin_ties():
    prof = _cap_lipid()
    o = polar.overlap(prof, 1, 2)
    for n in range(3):
        want = P.cover(prof[n, 1], prof[n, 2])
        assert {k: o[k][n] for k in want} == want, n
    assert (o['arc'][0], o['arc_max'][0], o['arc_start'][0]) == (50, 50, 350)
    assert (o['cover_min'][0], o['cover_argmin'][0]) == (9, 20)
    assert (o['arc'][1], o['arc_start'][1], o['cover_argmin'][1], o['cover_min'][1]) == (0, -1, -1, 0)
    back = polar.overlap(prof, 2, 1)                            # the other way round slice 1 overlaps everywhere
    assert back['arc'][1] == 90 and back['cover_min'][1] == 11 and back['arc'][0] == 0
    # LAST decides, not OUT: a second lipid run beyond the cap counts even if the first lies in front of it
    p2 = _prof(1)
    _put(p2, 0, 1, [7], 20, 25)
    _put(p2, 0, 2, [7], 3, 5, last=40)
    assert polar.overlap(p2, 1, 2)['arc'][0] == 1
    p2[0, 2, 7, LAST] = 25                                      # ends where the cap's run ends: not behind it
    assert polar.overlap(p2, 1, 2)['arc'][0] == 0
    with pytest.raises(ValueError):
        polar.overlap(prof, 1, 4)


def test_report_keys_values_and_json():
    prof = _cap_lipid()
    rep = polar.build_report(prof, 750, ['a', 'b', 'c'])
    assert list(rep) == ['ratio', 'images', 'classes', 'cap_over_lipid', 'thin_cap']
    assert rep['ratio'] == 112 and rep['images'] == ['a', 'b', 'c']
    assert json.loads(json.dumps(rep)) == rep
    cap, lipid = rep['classes']['Fibrous cap'], rep['classes']['Lipid core']
    assert list(cap) == ['slice', 'arc', 'arc_max', 'arc_start', 'depth_min', 'thickness_min', 'thickness_median', 'thickness_max']
    assert cap['slice'] == [0, 1] and cap['arc'] == [120, 90] and cap['arc_start'] == [300, 0]
    assert cap['depth_min'] == [4 / 112, 50 / 112] and cap['thickness_min'] == [9 / 112, 11 / 112]
    assert lipid['slice'] == [0, 1] and lipid['arc'] == [51, 90] and lipid['arc_max'] == [50, 90]
    assert rep['classes']['Lumen']['slice'] == [] and rep['classes']['Vasa vasorum']['slice'] == []
    col = rep['cap_over_lipid']
    assert col == {'slice': [0], 'arc': [50], 'arc_max': [50], 'arc_start': [350], 'cap_min': [9 / 112],
                   'cap_median': [P.cover(prof[0, 1], prof[0, 2])['cover_median'] / 112], 'cap_argmin': [20]}
    assert rep['thin_cap'] == {'max_cap': 0.065, 'min_arc': 90, 'slice': []}      # 9 / 112 = 0.080: not thin; arc 50: not wide
    flagged = polar.build_report(prof, 750, thin_cap=0.09, wide_arc=49)
    assert flagged['thin_cap'] == {'max_cap': 0.09, 'min_arc': 49, 'slice': [0]} and flagged['images'] == ['0', '1', '2']
    assert polar.build_report(prof, 750, thin_cap=0.09, wide_arc=50)['thin_cap']['slice'] == []      # strictly wider
    assert polar.build_report(prof, 750, thin_cap=9 / 112, wide_arc=49)['thin_cap']['slice'] == []    # strictly thinner
    swapped = polar.build_report(prof, 750, cap='Lipid core', lipid='Fibrous cap')
    assert swapped['cap_over_lipid']['slice'] == [1] and swapped['cap_over_lipid']['arc'] == [90]
    for v in list(cap.values()) + list(col.values()):
        assert all(type(x) in (int, float) for x in v)
    # a given ratio is used as it is; below 1 it is refused, as build_analysis refuses it
    assert polar.build_report(prof, 750, ratio=3)['classes']['Fibrous cap']['depth_min'][0] == 4 / 3
    with pytest.raises(ValueError, match='ratio'):
        polar.build_report(prof, 750, ratio=0)
    with pytest.raises(ValueError, match='ratio'):
        polar.build_report(prof, 6)                             # int(6 * 150 // 1000) == 0
    with pytest.raises(ValueError):
        polar.build_report(prof, 750, ['a'])
    with pytest.raises(ValueError):
        polar.build_report(prof, 750, cap='Plaque')
    # fewer channels than the cap / lipid pair: the per-class part still stands, the overlap is empty
    lumen_only = polar.build_report(prof[:, :1], 750)
    assert lumen_only['cap_over_lipid']['slice'] == [] and lumen_only['classes']['Fibrous cap']['slice'] == []


def test_carpet_view_paints_in_class_id_order():
    prof = _prof(3)
    _put(prof, 0, 0, range(0, 100), 1, 5)                       # Lumen
    _put(prof, 0, 2, range(50, 150), 8, 9)                      # Lipid core over it on 50..99
    _put(prof, 2, 1, range(340, 370), 8, 9)                     # Fibrous cap, wrapping
    _put(prof, 2, 3, [0], 1, 1)                                 # Vasa vasorum on top at degree 0
    img = polar.carpet_view(prof, ['Vasa vasorum', 'Lipid core', 'Lumen', 'Fibrous cap'])      # the order given does not matter
    assert img.shape == (360, 3, 3) and img.dtype == np.uint8
    assert (img[:, 1] == 128).all()
    assert tuple(img[10, 0]) == CLASS_COLORS_RGB['Lumen'] and tuple(img[60, 0]) == CLASS_COLORS_RGB['Lipid core']
    assert tuple(img[120, 0]) == CLASS_COLORS_RGB['Lipid core'] and tuple(img[200, 0]) == (128, 128, 128)
    assert tuple(img[350, 2]) == CLASS_COLORS_RGB['Fibrous cap'] and tuple(img[0, 2]) == CLASS_COLORS_RGB['Vasa vasorum']
    only = polar.carpet_view(prof, ['Lumen'])
    assert tuple(only[60, 0]) == CLASS_COLORS_RGB['Lumen'] and (only[:, 2] == 128).all()
    with pytest.raises(ValueError):
        polar.carpet_view(prof, ['Plaque'])
    with pytest.raises(ValueError):
        polar.carpet_view(prof[:, :2], ['Lipid core'])
    with pytest.raises(ValueError):
        polar.summarize(np.zeros((1, 4, 360), np.int32))


def test_abi_argument_checks_need_no_gpu():
    lib = L.lib()
    BAD_ARG = -5
    stack = (C.c_float * 64)(*([1.0] * 64))
    frames = (C.c_ubyte * 64)(*([7] * 64))
    pix = (C.c_int * (360 * 2))()
    length = (C.c_int * 360)()
    prof = (C.c_int * 64)(*([9] * 64))
    out = (C.c_ubyte * 64)(*([9] * 64))
    a = C.addressof

    def polar_call(stack=a(stack), N=1, H=4, W=4, SC=4, rp=a(pix), rl=a(length), R=1, prof=a(prof), map=a(out)):
        return lib.octseg_stack_polar(stack, N, H, W, SC, rp, rl, R, prof, map, None)

    def unwrap_call(frames=a(frames), N=1, H=4, W=4, ch=3, rp=a(pix), rl=a(length), R=1, out=a(out)):
        return lib.octseg_frames_unwrap(frames, N, H, W, ch, rp, rl, R, out, None)

    for kw in ({'stack': None}, {'rp': None}, {'rl': None}, {'prof': None}):
        assert polar_call(**kw) == BAD_ARG, kw
        assert b'null' in lib.octseg_last_error()
    for kw in ({'N': 0}, {'N': -1}, {'H': 0}, {'W': -1}, {'SC': 0}, {'SC': 9}, {'SC': 16}, {'R': -1}, {'H': 65536, 'W': 32768}):
        assert polar_call(**kw) == BAD_ARG, kw
    assert b'stack_polar' in lib.octseg_last_error()
    for kw in ({'frames': None}, {'rp': None}, {'rl': None}, {'out': None}):
        assert unwrap_call(**kw) == BAD_ARG, kw
        assert b'null' in lib.octseg_last_error()
    for kw in ({'N': 0}, {'H': -3}, {'W': 0}, {'ch': 0}, {'ch': 2}, {'ch': 4}, {'R': -1}, {'H': 32768, 'W': 65536}):
        assert unwrap_call(**kw) == BAD_ARG, kw
    assert b'frames_unwrap' in lib.octseg_last_error()
    assert list(prof) == [9] * 64 and list(out) == [9] * 64 and list(stack) == [1.0] * 64      # nothing was touched


def test_wrappers_refuse_bad_inputs_before_any_call():
    f32, u8 = torch.float32, torch.uint8
    with pytest.raises(ValueError, match='on the host'):
        polar.polar_profile(torch.zeros((1, 4, 4, 4), dtype=f32))
    with pytest.raises(ValueError, match='on the host'):
        polar.plaque_report(torch.zeros((1, 4, 4, 8), dtype=f32))
    with pytest.raises(ValueError, match='on the host'):
        polar.unwrap_frames(torch.zeros((1, 4, 4, 3), dtype=u8))
    for bad in (np.zeros((1, 4, 4, 4), np.float32), torch.zeros((1, 4, 4, 4), dtype=torch.float64), torch.zeros((1, 4, 4, 4), dtype=u8),
                torch.zeros((4, 4, 4), dtype=f32)):
        with pytest.raises(ValueError, match='must be a float32 CUDA tensor'):
            polar.polar_profile(bad)
    with pytest.raises(ValueError, match='at most 8 channels, got 9'):
        polar.polar_profile(torch.zeros((1, 4, 4, 9), dtype=f32))
    for shape in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, 0, 4), (1, 4, 4, 0)):
        with pytest.raises(ValueError, match='empty'):
            polar.polar_profile(torch.zeros(shape, dtype=f32))
        with pytest.raises(ValueError, match='empty'):
            polar.unwrap_frames(torch.zeros(shape, dtype=u8))
    for bad in (torch.zeros((1, 4, 4, 3), dtype=f32), torch.zeros((4, 4, 3), dtype=u8), np.zeros((1, 4, 4, 3), np.uint8)):
        with pytest.raises(ValueError, match='must be a uint8 CUDA tensor'):
            polar.unwrap_frames(bad)
    for ch in (2, 4):
        with pytest.raises(ValueError, match='1 or 3 channels'):
            polar.unwrap_frames(torch.zeros((1, 4, 4, ch), dtype=u8))
