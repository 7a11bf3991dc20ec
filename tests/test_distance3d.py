"""Surface distances of the volume without a GPU: the numpy restatement (tests/distance3d_ref.py) against scipy.ndimage by equality, the host
half of the volume functions of oct_segmentation_amd/distance.py, the ABI signatures, the refusals and the command line."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

import distance3d_ref as R3
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import distance

DEPTHS = [1, 2, 3, 9]
FRAMES = [(13, 70), (20, 130)]
STEPS = [1, 3, 50]


def scipy_edt2(target, s):
    d = ndimage.distance_transform_edt(~target, sampling=(s, 1, 1))
    d2 = d * d
    assert np.abs(d2 - np.rint(d2)).max() < 1e-6          # the rounding is safe: squared distances are integers
    return np.rint(d2).astype(np.int64)


def scipy_boundary(m):
    return m & ~ndimage.binary_erosion(m, ndimage.generate_binary_structure(3, 1), border_value=0)


# ---- 1. the restatement is scipy's answer
@pytest.mark.parametrize('h,w', FRAMES)
@pytest.mark.parametrize('n', DEPTHS)
def test_restated_boundary_and_transform_equal_scipy(n, h, w):
    m = R3.blob_volume(n, h, w, seed=1)
    b = R3.boundary(m)
    assert np.array_equal(b, scipy_boundary(m))
    assert m.any() and not m.all()
    if n >= 3:                                              # the erosion rule is exercised: a good share of the set voxels is NOT boundary
        assert (m & ~b).sum() >= 0.1 * m.sum(), ((m & ~b).sum(), m.sum())
        assert b[0].sum() == m[0].sum() and b[-1].sum() == m[-1].sum() and b[1].sum() < m[1].sum()
    else:                                                   # N <= 2: every set voxel is boundary
        assert np.array_equal(b, m)
    lone = np.zeros_like(m)                                 # a target in one slice only: every other slice is reached through z alone
    lone[n // 2] = m[n // 2]
    for s in STEPS:
        for t in (m, b, ~m, lone):
            assert np.array_equal(R3.edt2(t, s), scipy_edt2(t, s)), s


def test_restated_transform_equals_the_brute_force_minimum():
    m = R3.blob_volume(4, 6, 9, seed=2, count=1, size=0.5)
    assert m.any() and not m.all()
    zz, yy, xx = np.mgrid[:4, :6, :9]
    tz, ty, tx = np.nonzero(m)
    for s in (1, 3):
        want = (((zz[..., None] - tz) * s) ** 2 + (yy[..., None] - ty) ** 2 + (xx[..., None] - tx) ** 2).min(axis=-1)
        assert np.array_equal(R3.edt2(m, s), want)
    assert (R3.edt2(np.zeros((3, 4, 5), bool), 2) == R3.NONE).all() and R3.edt2(m, 1).dtype == np.int32
    full = np.ones((3, 4, 5), bool)
    shell = full.copy()
    shell[1, 1:-1, 1:-1] = False
    assert np.array_equal(R3.boundary(full), shell) and not R3.boundary(~full).any()


def test_restated_lists_minimum_and_counts():
    n, h, w, s = 3, 13, 70, 3
    a = np.stack([R3.blob_volume(n, h, w, 3), R3.blob_volume(n, h, w, 4, size=0.5)], axis=-1)
    b = np.stack([R3.blob_volume(n, h, w, 5), np.zeros((n, h, w), bool)], axis=-1)
    pairs = [(0, 0), (1, 0), (1, 1)]
    d2, off, tc = R3.directed(a, b, pairs, s=s)
    assert off.shape == (4,) and off[0] == 0 and off[-1] == d2.size and tc.shape == (3,) and tc[2] == 0
    want = scipy_edt2(scipy_boundary(b[..., 0]), s)
    for p, (ca, cb) in enumerate(pairs[:2]):
        assert np.array_equal(d2[off[p]:off[p + 1]], np.sort(want[scipy_boundary(a[..., ca])]))
    assert tc[0] == scipy_boundary(b[..., 0]).sum()
    assert (d2[off[2]:off[3]] == R3.NONE).all() and off[3] - off[2] == scipy_boundary(a[..., 1]).sum()
    keys = R3.pair_min(a, b, pairs, 'set', 'set', s)
    full = scipy_edt2(b[..., 0], s)
    q = a[..., 1]
    dmin = full[q].min()
    zs, ys, xs = np.nonzero(q & (full == dmin))
    assert int(keys[1]) == (int(dmin) << 32) | (int(zs[0]) * h * w + int(ys[0]) * w + int(xs[0]))
    assert int(keys[2]) >> 32 == R3.NONE and int(R3.pair_min(b, a, [(1, 0)])[0]) == 2 ** 64 - 1
    ov = R3.overlap(a, b, pairs)
    assert ov[0].tolist() == [int((a[..., 0] & b[..., 0]).sum()), int(a[..., 0].sum()), int(b[..., 0].sum())]


# ---- 2. build_volume_surface_metrics against a direct float64 computation
def test_volume_surface_metrics_from_the_reference_lists():
    n, h, w, s = 3, 13, 70, 3
    pred = np.stack([R3.blob_volume(n, h, w, 6), R3.blob_volume(n, h, w, 7), np.zeros((n, h, w), bool), np.zeros((n, h, w), bool)], axis=-1)
    truth = np.stack([R3.blob_volume(n, h, w, 8), np.zeros((n, h, w), bool), R3.blob_volume(n, h, w, 9), np.zeros((n, h, w), bool)], axis=-1)
    pairs, names = [(c, c) for c in range(4)], ['both', 'pred only', 'truth only', 'neither']
    ab, ba, ov = R3.directed(pred, truth, pairs, s=s), R3.directed(truth, pred, pairs, s=s), R3.overlap(pred, truth, pairs)
    for ratio, pct in ((None, 95), (4.0, 95), (None, 50)):
        rep = distance.build_volume_surface_metrics((ab[0], ba[0]), (ab[1], ba[1]), ov, names, ratio=ratio, percentile=pct)
        assert list(rep) == names
        scale = 1.0 if ratio is None else 1.0 / ratio
        for p, name in enumerate(names):
            a = np.sqrt(ab[0][ab[1][p]:ab[1][p + 1]].astype(np.float64))
            b = np.sqrt(ba[0][ba[1][p]:ba[1][p + 1]].astype(np.float64))
            col = rep[name]
            assert sorted(col) == sorted(['n_pred', 'n_truth', 'hd', 'hd95', 'assd', 'dice', 'iou'])
            assert col['n_pred'] == a.size == R3.boundary(pred[..., p]).sum() and col['n_truth'] == b.size
            if a.size and b.size:
                assert col['hd'] == float(max(a.max(), b.max()) * scale)
                assert col['hd95'] == float(max(np.percentile(a, pct), np.percentile(b, pct)) * scale)
                assert col['assd'] == float((a.sum() + b.sum()) / (a.size + b.size) * scale)
                assert 0 < col['assd'] <= col['hd'] and col['hd95'] <= col['hd']
            else:
                assert col['hd'] is None and col['hd95'] is None and col['assd'] is None
            inter, na, nb = (int(v) for v in ov[p])
            assert col['dice'] == (2.0 * inter / (na + nb) if na + nb else 1.0)
            assert col['iou'] == (inter / (na + nb - inter) if na + nb - inter else 1.0)
        json.dumps(rep)
    assert rep['both']['hd'] is not None and rep['pred only']['dice'] == 0.0 and rep['neither']['dice'] == 1.0
    with pytest.raises(ValueError):
        distance.build_volume_surface_metrics((ab[0], ba[0]), (ab[1], ba[1]), ov[None], names)
    with pytest.raises(ValueError):
        distance.build_volume_surface_metrics((ab[0], ba[0]), (ab[1], ba[1]), ov, names, ratio=0)


def test_a_lesion_one_slice_late_is_one_step_off():
    """What the per-slice report cannot say: the same square one slice later is exactly ``slice_step`` away everywhere."""
    a = np.zeros((4, 12, 12, 1), bool)
    b = np.zeros((4, 12, 12, 1), bool)
    a[1, 3:9, 3:9, 0] = True
    b[2, 3:9, 3:9, 0] = True
    ab, ba = R3.directed(a, b, [(0, 0)], s=7), R3.directed(b, a, [(0, 0)], s=7)
    rep = distance.build_volume_surface_metrics((ab[0], ba[0]), (ab[1], ba[1]), R3.overlap(a, b, [(0, 0)]), ['x'])['x']
    assert rep == {'n_pred': 36, 'n_truth': 36, 'hd': 7.0, 'hd95': 7.0, 'assd': 7.0, 'dice': 0.0, 'iou': 0.0}


def test_cap_distance_volume_from_the_packed_minimum():
    h, w = 13, 70
    key = (9 << 32) | (2 * h * w + 3 * w + 5)
    assert distance.build_cap_distance_volume(key, h, w) == {'distance': 3.0, 'at': (2, 3, 5), 'd2': 9}
    assert distance.build_cap_distance_volume(np.uint64(key), h, w, ratio=2)['distance'] == 1.5
    assert distance.build_cap_distance_volume(2 ** 64 - 1, h, w) is None
    assert distance.build_cap_distance_volume((distance.DIST_NONE << 32) | 7, h, w) is None
    with pytest.raises(ValueError):
        distance.build_cap_distance_volume(key, h, w, ratio=0)


# ---- 3. ABI
def test_symbols_of_the_volume_entry_points():
    i, p, z, ll = C.c_int, C.c_void_p, C.c_size_t, C.c_longlong
    pair = [p, p, i, i, i, i, i, p, i, i, i]
    want = {
        'octseg_volume_distance_scratch_bytes': (z, [i] * 7),
        'octseg_volume_boundary': (i, [p, i, i, i, i, p, z, p, p]),
        'octseg_volume_distance': (i, [p, i, i, i, i, i, i, p, z, p, p]),
        'octseg_volume_pair_distance_counts': (i, pair + [p, z, p, p, p]),
        'octseg_volume_pair_distance_keys': (i, pair + [i, p, z, ll, p, p, ll, p, p]),
        'octseg_volume_pair_distance_min': (i, pair + [i, p, z, p, p]),
    }
    header = open(os.path.join(os.path.dirname(__file__), '..', 'include', 'octseg.h')).read()
    for name, sig in want.items():
        assert L.SYMBOLS[name] == sig, name
        assert hasattr(L.lib(), name)
        assert name + '(' in header, name
    assert 'octseg_volume_boundary / octseg_volume_distance / octseg_volume_pair_distance_counts' in header          # the index comment


# ---- 4. refusals that need no GPU
def test_wrappers_refuse_before_the_device_is_asked():
    cpu = torch.zeros((3, 4, 4, 4))
    for bad in (1.5, 2.0, '2', None, True):
        with pytest.raises(ValueError, match='integer'):
            distance.check_slice_step(bad, 3)
        with pytest.raises(ValueError, match='integer'):
            distance.distance_volume(cpu, slice_step=bad)
        with pytest.raises(ValueError, match='integer'):
            distance.volume_surface_metrics(cpu, cpu, slice_step=bad)
    for bad in (0, -1, np.int64(0)):
        with pytest.raises(ValueError, match='at least 1'):
            distance.check_slice_step(bad, 3)
        with pytest.raises(ValueError, match='at least 1'):
            distance.cap_distance_volume(cpu, slice_step=bad)
    assert distance.check_slice_step(np.int32(3), 5) == 3 and distance.check_slice_step(32767, 2) == 32767 and distance.check_slice_step(10 ** 6, 1) == 10 ** 6
    assert distance.check_slice_step(81, 400) == 81                      # 81 * 399 = 32319
    with pytest.raises(ValueError, match='32767'):
        distance.check_slice_step(83, 400)                               # 83 * 399 = 33117
    with pytest.raises(ValueError, match='32767'):
        distance.check_slice_step(32768, 2)
    distance.check_volume(1024, 2048, 2048)
    with pytest.raises(ValueError, match='2\\^32'):
        distance.check_volume(1025, 2048, 2048)
    # mismatched stacks, an unknown part, a missing class name
    with pytest.raises(ValueError, match='must agree'):
        distance.directed_distances_volume(cpu, torch.zeros((2, 4, 4, 4)))
    with pytest.raises(ValueError, match='must agree'):
        distance.volume_surface_metrics(cpu, torch.zeros((3, 4, 5, 4)))
    with pytest.raises(ValueError, match='must agree'):
        distance.pair_minimum_volume(cpu, torch.zeros((3, 5, 4, 4)))
    for fn in (lambda: distance.distance_volume(cpu, to='edge'), lambda: distance.directed_distances_volume(cpu, cpu, src_part='surface'),
               lambda: distance.pair_minimum_volume(cpu, cpu, dst_part='inside')):
        with pytest.raises(ValueError, match='must be one of'):
            fn()
    with pytest.raises(ValueError, match="'Lipid core' has no channel"):
        distance.cap_distance_volume(cpu[..., :2])
    with pytest.raises(ValueError, match="'Calcium' has no channel"):
        distance.cap_distance_volume(cpu, lipid='Calcium')
    with pytest.raises(ValueError, match="'Lumen' has no channel"):
        distance.cap_distance_volume(cpu, classes=['a', 'b', 'Lipid core'])
    # with all of that in order, a host tensor is refused as the 2-D calls refuse it
    calls = (distance.boundary_volume, distance.distance_volume, lambda s: distance.directed_distances_volume(s, s),
             lambda s: distance.volume_surface_metrics(s, s), distance.cap_distance_volume, lambda s: distance.pair_minimum_volume(s, s))
    for bad in (cpu, cpu.double()):
        for fn in calls:
            with pytest.raises(ValueError, match='float32 CUDA tensor'):
                fn(bad)


def test_library_refuses_before_any_launch():
    lib = L.lib()
    size = lib.octseg_volume_distance_scratch_bytes
    assert size(1, 8, 4097, 1, 0, 0, 1) == 0 and size(1, 8, 8, 17, 0, 0, 1) == 0 and size(2, 8, 8, 1, 0, 0, 9) == 0 and size(2, 8, 8, 1, 0, 0, -1) == 0
    assert size(1025, 2048, 2048, 1, 0, 0, 1) == 0 and size(1024, 2048, 2048, 1, 0, 0, 1) > 0
    n, h, w, c = 9, 33, 65, 4
    words = h * 2
    flat, one, whole = size(n, h, w, c, 0, 0, 0), size(n, h, w, c, 0, 0, 1), size(n, h, w, c, 0, 0, h)
    assert flat >= 2 * n * c * words * 8                              # the raw planes and the part
    assert one >= flat + n * c * w * 6 and whole >= flat + n * c * h * w * 6      # 6 bytes per voxel of the band and channel
    assert whole <= flat + n * c * h * w * 6 + 1024 and size(n, h, w, c, 0, 0, 11) < whole
    assert size(n, h, w, c, c, 3, 0) >= flat + 2 * n * c * words * 8
    buf = (C.c_char * 4096)()                                # a host buffer: the calls below must return before they touch a pointer
    a = C.cast(buf, C.c_void_p)
    big = 1 << 40
    assert lib.octseg_volume_distance(a, 2, 8, 4097, 1, 0, 1, a, big, a, None) == -1
    assert lib.octseg_volume_distance(a, 2, 8, 8, 17, 0, 1, a, big, a, None) == -1
    assert lib.octseg_volume_distance(a, 2, 8, 8, 1, 3, 1, a, big, a, None) == -5
    for step in (0, -3, 32768):
        assert lib.octseg_volume_distance(a, 2, 8, 8, 1, 0, step, a, big, a, None) == -5
        assert b'slice_step' in lib.octseg_last_error()
    assert lib.octseg_volume_distance(a, 400, 8, 8, 1, 0, 83, a, big, a, None) == -5
    assert lib.octseg_volume_distance(a, 1025, 2048, 2048, 1, 0, 1, a, big, a, None) == -5 and b'2^32' in lib.octseg_last_error()
    need = size(2, 8, 8, 1, 0, 0, 1)
    assert lib.octseg_volume_distance(a, 2, 8, 8, 1, 0, 1, a, need - 1, a, None) == -5
    assert str(need).encode() in lib.octseg_last_error()              # the refusal names the bytes needed
    assert lib.octseg_volume_boundary(a, 2, 8, 8, 1, a, big, a, None) == -5            # out aliases the stack
    assert lib.octseg_volume_boundary(a, 2, 8, 8, 1, a, 16, None, None) == -5
    assert lib.octseg_volume_boundary(a, 2, 8, 8, 1, a, 16, C.c_void_p(C.addressof(buf) + 8), None) == -5 and b'scratch is smaller' in lib.octseg_last_error()
    assert lib.octseg_volume_pair_distance_counts(a, a, 2, 8, 8, 1, 1, a, 0, 2, 2, a, big, a, None, None) == -1
    assert lib.octseg_volume_pair_distance_counts(a, a, 2, 8, 8, 1, 1, a, 1, 2, 3, a, big, a, None, None) == -5
    assert lib.octseg_volume_pair_distance_keys(a, a, 2, 8, 8, 1, 1, a, 1, 2, 2, 1, a, big, 0, a, a, 0, a, None) == -5
    assert lib.octseg_volume_pair_distance_keys(a, a, 2, 8, 8, 1, 1, a, 1, 2, 2, 0, a, big, 0, a, a, 1, a, None) == -5
    assert lib.octseg_volume_pair_distance_keys(a, a, 2, 8, 8, 1, 1, a, 1, 2, 2, 1, a, big, 2 ** 31, a, a, 1, a, None) == -1
    assert lib.octseg_volume_pair_distance_min(a, a, 2, 8, 8, 1, 1, a, 1, 2, 2, 1, a, big, None, None) == -5
    assert lib.octseg_volume_pair_distance_min(a, a, 2, 8, 8, 1, 1, a, 1, 2, 2, 40000, a, big, a, None) == -5
    assert not any(buf.raw)


def test_volume_bands_follow_the_scratch_size_call():
    lib = L.lib()
    n, h, w = 9, 33, 65
    size = lambda rows: int(lib.octseg_volume_distance_scratch_bytes(n, h, w, 5, 0, 0, rows))
    assert distance.volume_bands(n, h, w, 5) == (h, 1, size(h))
    rows, bands, nbytes = distance.volume_bands(n, h, w, 5, scratch_bytes=size(7) + 5)
    assert (rows, bands, nbytes) == (7, 5, size(7))
    assert distance.volume_bands(n, h, w, 5, scratch_bytes=size(1)) == (1, h, size(1))
    with pytest.raises(ValueError, match=str(size(1))):
        distance.volume_bands(n, h, w, 5, scratch_bytes=size(1) - 1)
    with pytest.raises(ValueError, match='refuse'):
        distance.volume_bands(n, h, 4097, 5)


# ---- 5. the command line
def test_main_writes_the_volume_report_only_with_slice_step(tmp_path, monkeypatch):
    from PIL import Image
    import distance_ref as R
    pred_dir, truth_dir = tmp_path / 'pred', tmp_path / 'truth'
    pred_dir.mkdir()
    truth_dir.mkdir()
    n, h, w = 3, 20, 40
    vol = {'pred': np.stack([R3.blob_volume(n, h, w, 10 + c, size=0.6) for c in range(4)], axis=-1),
           'truth': np.stack([R3.blob_volume(n, h, w, 20 + c, size=0.6) for c in range(4)], axis=-1)}
    vol['pred'][..., 3] = False
    for folder, name in ((pred_dir, 'pred'), (truth_dir, 'truth')):
        for z, fname in enumerate(('s2.tiff', 's0.tiff', 's1.tiff')):        # written out of order: the slices are the sorted names
            Image.fromarray((vol[name][(z + 2) % 3] * 255).astype(np.uint8)).save(str(folder / fname))

    def lists2(pred, truth, pairs):
        ab, ba = R.directed(pred, truth, pairs), R.directed(truth, pred, pairs)
        return (ab[0], ba[0]), (ab[1], ba[1]), R.overlap(pred, truth, pairs)

    def lists3(pred, truth, pairs, s):
        ab, ba = R3.directed(pred, truth, pairs, s=s), R3.directed(truth, pred, pairs, s=s)
        return (ab[0], ba[0]), (ab[1], ba[1]), R3.overlap(pred, truth, pairs)
    monkeypatch.setattr(distance, '_host_surface_lists', lists2)
    monkeypatch.setattr(distance, '_host_volume_surface_lists', lists3)
    plain, stepped = tmp_path / 'plain', tmp_path / 'stepped'
    distance.main([str(pred_dir), str(truth_dir), str(plain)])
    distance.main([str(pred_dir), str(truth_dir), str(stepped), 'slice_step=4'])
    assert sorted(os.listdir(plain)) == ['surface_metrics.json']
    assert sorted(os.listdir(stepped)) == ['surface_metrics.json', 'surface_metrics_3d.json']
    assert open(plain / 'surface_metrics.json').read() == open(stepped / 'surface_metrics.json').read()
    saved = json.load(open(stepped / 'surface_metrics_3d.json'))
    names = ['Lumen', 'Fibrous cap', 'Lipid core', 'Vasa vasorum']
    assert saved['images'] == ['s0.tiff', 's1.tiff', 's2.tiff'] and saved['slice_step'] == 4 and saved['unit'] == 'pixel' and saved['classes'] == names
    pairs = [(c, c) for c in range(4)]
    want = distance.build_volume_surface_metrics(*lists3(vol['pred'], vol['truth'], pairs, 4), names)
    assert saved['metrics'] == json.loads(json.dumps(want))
    assert saved['metrics']['Lumen']['hd'] > 0 and saved['metrics']['Vasa vasorum']['hd'] is None
    for bad in ('slice_step=1.5', 'slice_step=0', 'slice_step=x'):
        with pytest.raises((SystemExit, ValueError)):
            distance.main([str(pred_dir), str(truth_dir), str(tmp_path / 'bad'), bad])
    assert not os.path.exists(tmp_path / 'bad')
    with pytest.raises(SystemExit):
        distance.main([str(pred_dir), 'slice_step=2'])
