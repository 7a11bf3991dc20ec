"""Boundary distances without a GPU: the numpy restatement (tests/distance_ref.py) against scipy.ndimage by equality, the host half of
oct_segmentation_amd/distance.py on designed cases, the ABI signatures, the refusals and the command line."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

import distance_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import distance

SHAPES = [(1, 1), (1, 70), (70, 1), (33, 65), (64, 64), (97, 130)]
DENSITIES = [0.001, 0.02, 0.5]


def drawn(h, w, density, seed=0):
    """A seeded boolean plane at the density, one pixel forced when the draw is empty."""
    rng = np.random.RandomState(seed + 7919 * h + 31 * w + int(density * 1e4))
    m = rng.rand(h, w) < density
    if not m.any():
        m[rng.randint(h), rng.randint(w)] = True
    return m


def scipy_edt2(target):
    d = ndimage.distance_transform_edt(~target)
    d2 = d * d
    assert np.abs(d2 - np.rint(d2)).max() < 1e-9          # the rounding is safe: squared distances are integers
    return np.rint(d2).astype(np.int64)


def scipy_boundary(m):
    return m & ~ndimage.binary_erosion(m, ndimage.generate_binary_structure(2, 1), border_value=0)


# ---- 1. the restatement is scipy's answer
@pytest.mark.parametrize('density', DENSITIES)
@pytest.mark.parametrize('h,w', SHAPES)
def test_restated_transform_equals_scipy(h, w, density):
    m = drawn(h, w, density)
    assert np.array_equal(R.edt2(m), scipy_edt2(m))
    assert np.array_equal(R.boundary(m), scipy_boundary(m))
    b = R.boundary(m)
    assert np.array_equal(R.edt2(b), scipy_edt2(b))
    if not m.all():
        assert np.array_equal(R.edt2(~m), scipy_edt2(~m))
    else:                                                   # scipy's answer for an empty target is meaningless: NONE by rule
        assert (R.edt2(~m) == R.NONE).all()


def test_restated_empty_target_and_full_plane():
    z = np.zeros((5, 9), bool)
    assert (R.edt2(z) == R.NONE).all() and R.edt2(z).dtype == np.int32
    full = np.ones((5, 9), bool)
    ring = np.ones((5, 9), bool)
    ring[1:-1, 1:-1] = False
    assert np.array_equal(R.boundary(full), ring) and np.array_equal(scipy_boundary(full), ring)
    assert not R.boundary(z).any()


def test_restated_lists_minimum_and_counts():
    a = np.stack([drawn(33, 65, 0.02, 1), drawn(33, 65, 0.5, 2)], axis=-1)[None]
    b = np.stack([drawn(33, 65, 0.02, 3), np.zeros((33, 65), bool)], axis=-1)[None]
    pairs = [(0, 0), (1, 0), (1, 1)]
    d2, off, tc = R.directed(a, b, pairs)
    assert off.tolist()[0] == 0 and off[-1] == d2.size and tc.shape == (1, 3) and tc[0, 2] == 0
    want = scipy_edt2(R.boundary(b[0, :, :, 0]))
    for s, (ca, cb) in enumerate(pairs[:2]):
        q = R.boundary(a[0, :, :, ca])
        assert np.array_equal(d2[off[s]:off[s + 1]], np.sort(want[q]))
    assert (d2[off[2]:off[3]] == R.NONE).all() and off[3] - off[2] == R.boundary(a[0, :, :, 1]).sum()
    keys = R.pair_min(a, b, pairs, 'set', 'set')
    full = scipy_edt2(b[0, :, :, 0] != 0)
    q = a[0, :, :, 0]
    dmin = full[q].min()
    ys, xs = np.nonzero(q & (full == dmin))
    assert int(keys[0, 0]) == (int(dmin) << 32) | (int(ys[0]) * 65 + int(xs[0]))
    assert int(keys[0, 2]) >> 32 == R.NONE
    assert int(R.pair_min(b, a, [(1, 0)])[0, 0]) == 2 ** 64 - 1
    ov = R.overlap(a, b, pairs)
    assert ov[0, 0].tolist() == [int((a[0, :, :, 0] & b[0, :, :, 0]).sum()), int(a[0, :, :, 0].sum()), int(b[0, :, :, 0].sum())]


# ---- 2. build_surface_metrics on hand-made integer lists
def squares():
    """Concentric axis-aligned squares of sides 20 and 30 in a 50 x 50 frame, and their directed lists DERIVED BY HAND: every boundary pixel of the
    small square is 5 from the large one's boundary; a boundary pixel of the large square is 5 from the small one's where it faces a side (20 per
    side), and sqrt(25 + k^2) from the nearest corner where it overhangs by k = 1..5 (k = 5: the four corners, once each; k < 5: twice per corner)."""
    a = np.zeros((50, 50), bool)
    b = np.zeros((50, 50), bool)
    a[15:35, 15:35] = True
    b[10:40, 10:40] = True
    d_ab = [25] * 76
    d_ba = sorted([25] * 80 + [26] * 8 + [29] * 8 + [34] * 8 + [41] * 8 + [50] * 4)
    return a, b, d_ab, d_ba


def test_surface_metrics_of_concentric_squares():
    """The statistics are numpy calls on the integers, the same calls any reference would make: comparing them to a reference only checks
    plumbing.  What pins their DEFINITION are these designed cases, whose lists and answers are derived by hand."""
    a, b, d_ab, d_ba = squares()
    # the restatement produces the hand-derived lists
    got_ab = R.directed(a[None, :, :, None], b[None, :, :, None], [(0, 0)])
    got_ba = R.directed(b[None, :, :, None], a[None, :, :, None], [(0, 0)])
    assert got_ab[0].tolist() == d_ab and got_ba[0].tolist() == d_ba
    rep = distance.build_surface_metrics((d_ab, d_ba), ([0, 76], [0, 116]), [[[400, 400, 900]]], ['Lumen'])['Lumen']
    assert rep['slice'] == [0] and rep['n_pred'] == [76] and rep['n_truth'] == [116]
    assert rep['hd'][0] == pytest.approx(math.sqrt(50), abs=1e-12)
    # 116 sorted values, rank 0.95 * 115 = 109.25: entries 109 and 110 are both sqrt(41) (80 + 3 * 8 = 104 values lie below them)
    assert rep['hd95'][0] == pytest.approx(math.sqrt(41), abs=1e-12)
    total = 76 * 5 + 80 * 5 + 8 * (math.sqrt(26) + math.sqrt(29) + math.sqrt(34) + math.sqrt(41)) + 4 * math.sqrt(50)
    assert rep['assd'][0] == pytest.approx(total / (76 + 116), abs=1e-12)
    assert rep['dice'][0] == pytest.approx(800 / 1300) and rep['iou'][0] == pytest.approx(400 / 900)
    # ratio divides the three distances and nothing else
    rep4 = distance.build_surface_metrics((d_ab, d_ba), ([0, 76], [0, 116]), [[[400, 400, 900]]], ['Lumen'], ratio=4)['Lumen']
    for k in ('hd', 'hd95', 'assd'):
        assert rep4[k][0] == pytest.approx(rep[k][0] / 4, abs=1e-12)
    assert rep4['dice'] == rep['dice'] and rep4['n_pred'] == rep['n_pred']
    # the percentile is a parameter: the 50th of both sides is 5
    assert distance.build_surface_metrics((d_ab, d_ba), ([0, 76], [0, 116]), [[[400, 400, 900]]], ['Lumen'], percentile=50)['Lumen']['hd95'] == [5.0]


def test_surface_metrics_of_single_pixels_and_empty_sides():
    # slice 0: (2, 3) against (5, 7): 3-4-5.  slice 1: the truth is empty.  slice 2: both are empty.
    rep = distance.build_surface_metrics(([25, distance.DIST_NONE], [25]), ([0, 1, 2, 2], [0, 1, 1, 1]),
                                         [[[0, 1, 1]], [[0, 1, 0]], [[0, 0, 0]]], ['x'])['x']
    assert rep['slice'] == [0, 1, 2] and rep['n_pred'] == [1, 1, 0] and rep['n_truth'] == [1, 0, 0]
    assert rep['hd'] == [5.0, None, None] and rep['hd95'] == [5.0, None, None] and rep['assd'] == [5.0, None, None]
    assert rep['dice'] == [0.0, 0.0, 1.0] and rep['iou'] == [0.0, 0.0, 1.0]          # zero_division = 1.0, as metrics.py
    json.dumps(rep)
    with pytest.raises(ValueError):
        distance.build_surface_metrics(([25], [25]), ([0, 1], [0, 2]), [[[0, 1, 1]]], ['x'])
    with pytest.raises(ValueError):
        distance.build_surface_metrics(([25], [25]), ([0, 1], [0, 1]), [[[0, 1, 1]]], ['x'], ratio=0)


def test_cap_distance_from_packed_minima():
    keys = np.array([(9 << 32) | (3 * 70 + 5), 2 ** 64 - 1, (distance.DIST_NONE << 32) | 7, (1 << 32) | 0], np.uint64)
    rep = distance.build_cap_distance(keys, 70)
    assert rep == {'slice': [0, 3], 'distance': [3.0, 1.0], 'at': [(3, 5), (0, 0)], 'd2': [9, 1]}
    assert distance.build_cap_distance(keys, 70, ratio=2)['distance'] == [1.5, 0.5]


# ---- 3. ABI
def test_symbols_of_the_distance_entry_points():
    i, p, z, ll = C.c_int, C.c_void_p, C.c_size_t, C.c_longlong
    pair = [p, p, i, i, i, i, i, p, i, i, i, p, z]
    want = {
        'octseg_distance_scratch_bytes': (z, [i] * 6),
        'octseg_stack_boundary': (i, [p, i, i, i, i, p, z, p, p]),
        'octseg_stack_distance': (i, [p, i, i, i, i, i, p, z, p, p]),
        'octseg_pair_distance_counts': (i, pair + [p, p, p]),
        'octseg_pair_distance_keys': (i, pair + [ll, p, p, ll, p, p]),
        'octseg_pair_distance_min': (i, pair + [p, p]),
    }
    for name, sig in want.items():
        assert L.SYMBOLS[name] == sig, name
        assert hasattr(L.lib(), name)
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'octseg.h')).read()
    assert '#define OCTSEG_DIST_NONE 0x7fffffff' in header and distance.DIST_NONE == 0x7fffffff == R.NONE


# ---- 4. refusals that need no GPU
def test_wrappers_refuse_host_tensors_and_oversized_extents():
    cpu = torch.zeros((1, 4, 4, 4))
    calls = (distance.boundary_stack, distance.distance_stack, lambda s: distance.directed_distances(s, s),
             lambda s: distance.surface_metrics(s, s), distance.cap_distance)
    for bad in (cpu, cpu.numpy(), cpu.double(), cpu[0]):
        for fn in calls:
            with pytest.raises(ValueError, match='float32 CUDA tensor'):
                fn(bad)
    with pytest.raises(ValueError, match='4096'):
        distance.check_extents(1, 8, 4097, 4)
    with pytest.raises(ValueError, match='4096'):
        distance.check_extents(1, 4097, 8, 4)
    with pytest.raises(ValueError, match='at most 16 channels'):
        distance.check_extents(1, 8, 8, 17)
    with pytest.raises(ValueError):
        distance.check_extents(0, 8, 8, 1)
    with pytest.raises(ValueError):
        distance.check_extents(2 ** 27, 8, 8, 16, 16)
    distance.check_extents(186, 4096, 4096, 16, 256)
    with pytest.raises(ValueError):
        distance.distance_stack(cpu, to='edge')


def test_library_refuses_before_any_launch():
    lib = L.lib()
    assert lib.octseg_distance_scratch_bytes(1, 8, 4097, 1, 0, 0) == 0 and lib.octseg_distance_scratch_bytes(1, 8, 8, 17, 0, 0) == 0
    need = lib.octseg_distance_scratch_bytes(2, 33, 65, 4, 0, 0)
    words = 33 * 2
    assert need >= 2 * 4 * (2 * words * 8 + 33 * 65 * 2) and lib.octseg_distance_scratch_bytes(2, 33, 65, 4, 4, 3) >= need + 2 * 2 * 4 * words * 8
    buf = (C.c_char * 4096)()                                # a host buffer: the calls below must return before they touch a pointer
    a = C.cast(buf, C.c_void_p)
    big = 1 << 40
    assert lib.octseg_stack_distance(a, 1, 8, 4097, 1, 0, a, big, a, None) == -1
    assert lib.octseg_stack_distance(a, 1, 8, 8, 17, 0, a, big, a, None) == -1
    assert lib.octseg_stack_distance(a, 1, 8, 8, 1, 3, a, big, a, None) == -5
    assert lib.octseg_stack_distance(a, 1, 8, 8, 1, 0, a, 16, a, None) == -5
    assert b'scratch is smaller' in lib.octseg_last_error()
    assert lib.octseg_stack_boundary(a, 1, 8, 8, 1, a, big, a, None) == -5          # out aliases the stack
    assert lib.octseg_stack_boundary(a, 0, 8, 8, 1, a, big, None, None) == -5
    assert lib.octseg_pair_distance_counts(a, a, 1, 8, 8, 1, 1, a, 0, 2, 2, a, big, a, None, None) == -1
    assert lib.octseg_pair_distance_counts(a, a, 1, 8, 8, 1, 1, a, 1, 2, 3, a, big, a, None, None) == -5
    assert lib.octseg_pair_distance_keys(a, a, 1, 8, 8, 1, 1, a, 1, 2, 2, a, big, 0, a, a, 0, a, None) == -5
    assert lib.octseg_pair_distance_keys(a, a, 1, 8, 8, 1, 1, a, 1, 2, 2, a, big, 2 ** 31, a, a, 1, a, None) == -1
    assert lib.octseg_pair_distance_min(a, a, 1, 8, 8, 1, 1, a, 1, 2, 2, a, big, None, None) == -5
    assert not any(buf.raw)


# ---- 5. the command line
def test_main_on_two_tiff_directories(tmp_path, monkeypatch):
    from PIL import Image
    pred_dir, truth_dir, save_dir = tmp_path / 'pred', tmp_path / 'truth', tmp_path / 'out'
    pred_dir.mkdir()
    truth_dir.mkdir()
    a, b, d_ab, d_ba = squares()
    masks = {}
    for name, planes in (('s0.tiff', (a, b)), ('s1.tiff', (b, b))):
        for folder, m in zip((pred_dir, truth_dir), planes):
            arr = np.zeros((50, 50, 4), np.uint8)
            arr[:, :, 0] = m * 255
            arr[:, :, 2] = drawn(50, 50, 0.02, len(masks)) * 255
            Image.fromarray(arr).save(str(folder / name))
            masks[(folder.name, name)] = arr
    Image.fromarray(np.zeros((50, 50, 4), np.uint8)).save(str(pred_dir / 'unpaired.tiff'))

    def lists(pred, truth, pairs):                           # what the GPU would return, from the restatement
        ab, ba = R.directed(pred, truth, pairs), R.directed(truth, pred, pairs)
        return (ab[0], ba[0]), (ab[1], ba[1]), R.overlap(pred, truth, pairs)
    monkeypatch.setattr(distance, '_host_surface_lists', lists)
    report = distance.main([str(pred_dir), str(truth_dir), str(save_dir)])
    saved = json.load(open(save_dir / 'surface_metrics.json'))
    assert saved == json.loads(json.dumps(report))
    assert saved['images'] == ['s0.tiff', 's1.tiff'] and saved['classes'] == ['Lumen', 'Fibrous cap', 'Lipid core', 'Vasa vasorum']
    lumen = saved['metrics']['Lumen']
    assert lumen['n_pred'] == [76, 116] and lumen['n_truth'] == [116, 116]
    assert lumen['hd'][0] == pytest.approx(math.sqrt(50)) and lumen['hd95'][0] == pytest.approx(math.sqrt(41))
    assert lumen['hd'][1] == 0.0 and lumen['assd'][1] == 0.0 and lumen['dice'][1] == 1.0
    assert saved['metrics']['Fibrous cap']['hd'] == [None, None] and saved['metrics']['Fibrous cap']['dice'] == [1.0, 1.0]
    want = distance.build_surface_metrics(*lists(np.stack([masks[('pred', 's0.tiff')], masks[('pred', 's1.tiff')]]),
                                                 np.stack([masks[('truth', 's0.tiff')], masks[('truth', 's1.tiff')]]), [(2, 2)]), ['Lipid core'])
    assert saved['metrics']['Lipid core'] == json.loads(json.dumps(want['Lipid core']))
    with pytest.raises(SystemExit):
        distance.main([str(pred_dir)])
