"""CPU tests of the pullback measurements (oct_segmentation_amd/analysis.py): the ray table against upstream's formula, the numpy restatement
of the kernel (tests/analysis_ref.py) against what the reference's own calculate_object_thickness and get_analysis returned on an excerpt of
its demo pullback (tests/golden/pullback_demo_excerpt.npz), and build_analysis from the restatement's integers against the same record.
Integers and the float64 arithmetic on them are compared for equality."""
import json
import math
import os

import numpy as np
import pytest

import analysis_ref as R
from oct_segmentation_amd import analysis
from oct_segmentation_amd.model import CLASS_IDS

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, 'golden', 'pullback_demo_excerpt.npz')
SHAPES = [(1, 1), (2, 3), (5, 4), (17, 33), (64, 48), (31, 31)]
_measured = {}


def _fixture_measured():
    """counts and radii of the fixture's stack by the restatement, computed once."""
    if 'm' not in _measured:
        _measured['m'] = R.measure(R.load_fixture(FIXTURE)['stack'])
    return _measured['m']


@pytest.mark.parametrize('h,w', SHAPES + [(750, 750)])
def test_ray_table_is_the_formula(h, w):
    pix, length = analysis.ray_table(h, w)
    max_radius = int(math.sqrt(w ** 2 + h ** 2)) // 2
    assert pix.dtype == length.dtype == np.int32 and pix.shape == (360, max(max_radius - 1, 0)) and length.shape == (360,)
    for angle in range(0, 360, 1 if h * w < 5000 else 7):
        rad = math.radians(angle)
        n = 0
        for r in range(1, max_radius):
            x, y = int(w // 2 + r * math.cos(rad)), int(h // 2 + r * math.sin(rad))
            if not (0 <= x < w and 0 <= y < h):
                break
            assert pix[angle, n] == y * w + x, (angle, r)
            n += 1
        assert length[angle] == n, angle
        assert not pix[angle, n:].any()
    assert np.array_equal(length, R.ray_lengths(h, w))
    if (h, w) == (1, 1):
        assert pix.shape[1] == 0


def test_truncation_toward_zero_keeps_coordinates_in_minus_one_to_zero_inside():
    # 5 x 4: centre (2, 2), max_radius 3, R = 2.  At 135 degrees r = 2 gives x = int(2 - 1.414) = 0 and y = int(2 + 1.414) = 3, inside;
    # at 225 degrees r = 2 gives int(2 - 1.414) = 0 on both axes
    pix, length = analysis.ray_table(5, 4)
    assert pix.shape == (360, 2)
    assert length[225] == 2 and pix[225, 1] == 0
    # 1 x 9: centre (4, 0); at 350 degrees y = int(0 - r * 0.17) = int(-0.17 ...) = 0 stays inside for r = 1..3
    pix, length = analysis.ray_table(1, 9)
    assert length[350] == 3 and list(pix[350, :3]) == [4, 5, 6]      # int(4 + 0.98) = 4, int(4 + 1.97) = 5, int(4 + 2.95) = 6


def test_restatement_equals_the_references_thickness_function():
    fx = R.load_fixture(FIXTURE)
    counts, radii = _fixture_measured()
    assert len(fx['thickness']) == 91
    for (s, c), want in fx['thickness'].items():
        got = analysis.radial_thickness(radii[s, c])
        assert got['all_measurements'] == want['all_measurements'], (s, c)
        assert got['median'] == want['median'] and got['min'] == want['min'] and got['max'] == want['max'], (s, c)
    assert np.array_equal(counts, fx['stack'].reshape(48, -1, 4).sum(axis=1))


def test_build_analysis_equals_the_references_get_analysis():
    fx = R.load_fixture(FIXTURE)
    counts, radii = _fixture_measured()
    rec = fx['recorded']
    data = analysis.build_analysis(counts, radii, 750, 750, fx['names'])
    assert data['ratio'] == rec['ratio'] == 112 and data['images'] == rec['images']
    assert list(data['objects']) == list(rec['objects']) == list(CLASS_IDS)
    present = 0
    for cl, want in rec['objects'].items():
        got = data['objects'][cl]
        for k in ('slice', 'area', 'object_id', 'img_name'):
            assert got[k] == want[k], (cl, k)
        assert got['masks'] == []
        ch = CLASS_IDS[cl] - 1
        for i, s in enumerate(want['slice']):
            t = fx['thickness'][(s, ch)]
            assert got['thickness_mean'][i] == t['median'] / rec['ratio']
            assert got['thickness_min'][i] == t['min'] / rec['ratio']
            assert got['thickness_max'][i] == t['max'] / rec['ratio']
        present += len(want['slice'])
    assert present == len(fx['thickness'])
    # the excerpt has what the run rule is about: more than one object per class, runs longer than one slice
    assert max(rec['objects']['Fibrous cap']['object_id']) >= 2 and max(rec['objects']['Vasa vasorum']['object_id']) >= 2
    assert rec['objects']['Lumen']['object_id'] == [0] * 48
    back = json.loads(json.dumps(data))
    assert back == data


def test_radial_thickness_dict():
    assert analysis.radial_thickness(np.zeros(360, np.int32)) == {'median': 0, 'min': 0, 'max': 0, 'all_measurements': []}
    row = np.zeros(360, np.int32)
    row[[3, 10, 200, 359]] = [7, 2, 9, 4]
    t = analysis.radial_thickness(row)
    assert t == {'median': 5.5, 'min': 2, 'max': 9, 'all_measurements': [7, 2, 9, 4]}
    assert type(t['median']) is float and type(t['min']) is int


def test_run_rule_full_mask_quirk_and_ratio():
    h, w = 20, 10
    counts = np.zeros((7, 4), np.int32)
    radii = np.zeros((7, 4, 360), np.int32)
    counts[:, 0] = [5, 9, 0, 200, 4, 4, 1]            # slice 3 is completely full: absent, and it splits the run
    counts[:, 3] = [0, 0, 1, 0, 1, 0, 199]
    radii[0, 0, :4] = [3, 5, 1, 1]
    names = list('abcdefg')
    d = analysis.build_analysis(counts, radii, h, w, names)
    assert d['ratio'] == 3                             # int(20 * 150 // 1000)
    lumen, vv = d['objects']['Lumen'], d['objects']['Vasa vasorum']
    assert lumen['slice'] == [0, 1, 4, 5, 6] and lumen['object_id'] == [0, 0, 1, 1, 1]
    assert lumen['area'] == [pow(5 // 3, 0.5), pow(9 // 3, 0.5), 1.0, 1.0, 0.0]
    assert lumen['img_name'] == ['a', 'b', 'e', 'f', 'g']
    assert lumen['thickness_mean'][0] == 2.0 / 3 and lumen['thickness_min'][0] == 1 / 3 and lumen['thickness_max'][0] == 5 / 3
    assert lumen['thickness_mean'][1:] == [0.0] * 4
    assert vv['slice'] == [2, 4, 6] and vv['object_id'] == [0, 1, 2]
    assert d['objects']['Fibrous cap']['slice'] == [] and d['images'] == names
    assert analysis.build_analysis(counts, radii, h, w, names, ratio=1)['objects']['Lumen']['area'][1] == 3.0
    json.dumps(d)
    with pytest.raises(ValueError):
        analysis.build_analysis(counts, radii, 6, 10, names)          # default ratio int(6 * 150 // 1000) = 0
    with pytest.raises(ValueError):
        analysis.build_analysis(counts, radii, h, w, names, ratio=0)
    with pytest.raises(ValueError):
        analysis.build_analysis(counts, radii, h, w, names[:3])
    with pytest.raises(ValueError):
        analysis.build_analysis(counts, radii[:, :, :100], h, w, names)


def test_contour_thickness_is_refused_with_a_reason():
    with pytest.raises(NotImplementedError, match='findContours'):
        analysis.analyze_stack(None, thickness='contour')
    with pytest.raises(ValueError):
        analysis.analyze_stack(None, thickness='chord')
    with pytest.raises(ValueError):
        analysis.measure_stack(np.zeros((1, 4, 4, 4), np.float32))    # not a CUDA tensor


def test_restatement_walk_rule():
    v = lambda s: np.array([ch == '1' for ch in s])                  # noqa: E731
    assert R.walk(v('')) == 0 and R.walk(v('0000')) == 0
    assert R.walk(v('1')) == 1 and R.walk(v('1111')) == 4
    assert R.walk(v('0011100')) == 5 and R.walk(v('0011101')) == 5     # gap before skipped, first gap after ends the ray
    assert R.walk(v('10')) == 1 and R.walk(v('0001')) == 4
