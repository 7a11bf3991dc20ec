"""Surface distances of the volume on the GPU (the octseg_volume_* calls of csrc/distance.hip through oct_segmentation_amd/distance.py) against
the numpy restatement of tests/distance3d_ref.py, which tests/test_distance3d.py holds to scipy.ndimage.  Every comparison is integer equality:
there is no tolerance."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import distance3d_ref as R3
from analysis_ref import load_fixture
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import distance

pytestmark = pytest.mark.gpu

DEPTHS = [1, 2, 3, 9]
FRAMES = [(1, 70), (13, 70), (33, 65), (20, 130)]       # a word boundary, H no multiple of the column pass's 8 rows, a one-row frame
STEPS = [1, 3, 50]
PARTS = ('set', 'clear', 'boundary')
# (source channel, target channel) over the five channels of blob_stack: sparse, dense, one slice only, empty, full -- an empty query, an empty
# target, and a channel against itself are all among them (the pair list of tests/test_gpu_distance.py)
PAIRS = [(0, 1), (1, 0), (2, 2), (3, 2), (2, 3), (4, 4), (2, 4), (1, 2)]
FIXTURE = os.path.join(os.path.dirname(__file__), 'golden', 'pullback_demo_excerpt.npz')


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()        # a copy: the cached stacks are read-only


def host(t):
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def blob_stack(n, h, w):
    """[n, h, w, 5]: a sparse blob, a dense blob, a blob present in one slice only, an empty and a full channel.  Read-only."""
    st = np.zeros((n, h, w, 5), np.float32)
    st[..., 0] = R3.blob_volume(n, h, w, 1, count=1, size=0.4)
    st[..., 1] = R3.blob_volume(n, h, w, 2, count=4)
    st[n // 2, :, :, 2] = R3.blob_volume(n, h, w, 3, count=2, size=0.6)[n // 2]
    st[..., 4] = 1.0
    assert st[..., 0].any() and st[..., 2].any() and st[..., 0].sum() < st[..., 1].sum() <= st[..., 4].sum()
    st.setflags(write=False)
    return st


@functools.lru_cache(maxsize=None)
def ref_maps(n, h, w, s):
    st = blob_stack(n, h, w)
    return {p: R3.distance_volume(st, p, s) for p in PARTS}


@functools.lru_cache(maxsize=None)
def ref_lists(n, h, w, src_part, dst_part, s):
    st = blob_stack(n, h, w)
    return R3.directed(st, st, PAIRS, src_part, dst_part, s), R3.pair_min(st, st, PAIRS, src_part, dst_part, s), R3.overlap(st, st, PAIRS)


def misaligned(a):
    """The stack as a contiguous CUDA view whose base is 4 bytes off 16-byte alignment."""
    flat = torch.empty((a.size + 1,), dtype=torch.float32, device='cuda')
    view = flat[1:].view(a.shape)
    view.copy_(torch.from_numpy(np.array(a, dtype=np.float32)))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    return view


def lists_equal(got, want):
    (d2, off, tc), (wd2, woff, wtc) = got, want
    return d2.dtype == np.int64 and np.array_equal(d2, wd2) and np.array_equal(off, woff) and np.array_equal(tc, wtc)


# ---- 1. boundary and maps
@pytest.mark.parametrize('h,w', FRAMES)
@pytest.mark.parametrize('n', DEPTHS)
def test_boundary_and_maps_equal_the_restatement(n, h, w):
    st = blob_stack(n, h, w)
    d = dev(st)
    before = d.clone()
    edge = distance.boundary_volume(d)
    assert edge.dtype == torch.float32 and edge.shape == d.shape
    assert np.array_equal(host(edge), R3.boundary_volume(st))
    for s in STEPS:
        want = ref_maps(n, h, w, s)
        for part in PARTS:
            got = distance.distance_volume(d, to=part, slice_step=s)
            assert got.dtype == torch.int32 and tuple(got.shape) == (n, 5, h, w)
            assert np.array_equal(host(got), want[part]), (part, s)
    assert (host(distance.distance_volume(d, to='set'))[:, 3] == distance.DIST_NONE).all()        # the empty channel
    assert torch.equal(d, before)                                        # the input stack is never modified


def test_four_channels_and_a_misaligned_base():
    n, h, w, s = 3, 33, 65, 3
    st = blob_stack(n, h, w)
    want, edge = ref_maps(n, h, w, s), R3.boundary_volume(st)
    for d, cs in ((dev(st[..., :4]), slice(0, 4)), (misaligned(st[..., 1:5]), slice(1, 5)), (dev(st[..., 2:3]), slice(2, 3))):
        assert np.array_equal(host(distance.boundary_volume(d)), edge[..., cs])
        for part in PARTS:
            assert np.array_equal(host(distance.distance_volume(d, to=part, slice_step=s)), want[part][:, cs]), part


# ---- 2. degenerate identities
def test_one_slice_is_the_per_slice_map_whatever_the_step():
    d = dev(blob_stack(1, 33, 65))
    for part in ('set', 'clear'):
        flat = distance.distance_stack(d, to=part)
        for s in (1, 50, 32767):
            assert torch.equal(distance.distance_volume(d, to=part, slice_step=s), flat)
    # with one slice every set voxel is boundary (both ends are outside the volume), so the 3-D boundary is the set part, not the 2-D ring
    assert torch.equal(distance.distance_volume(d, to='boundary', slice_step=3), distance.distance_stack(d, to='set'))
    assert not torch.equal(distance.distance_stack(d, to='boundary'), distance.distance_stack(d, to='set'))


def test_far_apart_slices_are_the_per_slice_maps():
    n, h, w = 3, 13, 70
    st = blob_stack(n, h, w)[..., :2]
    assert all(st[z, :, :, c].any() for z in range(n) for c in range(2))
    s = 72
    assert s * s > h * h + w * w
    d = dev(st)
    assert torch.equal(distance.distance_volume(d, to='set', slice_step=s), distance.distance_stack(d, to='set'))


def test_a_single_voxel_in_the_first_slice_is_the_closed_form():
    """The worst case of the search along z: every voxel of the last slice walks the whole stack."""
    n, h, w = 9, 13, 70
    st = np.zeros((n, h, w, 1), np.float32)
    st[0, 4, 66, 0] = 1
    zz, yy, xx = np.mgrid[:n, :h, :w]
    got = host(distance.distance_volume(dev(st), to='set', slice_step=1))[:, 0]
    assert np.array_equal(got, zz ** 2 + (yy - 4) ** 2 + (xx - 66) ** 2)
    got = host(distance.distance_volume(dev(st), to='boundary', slice_step=7))[:, 0]
    assert np.array_equal(got, (7 * zz) ** 2 + (yy - 4) ** 2 + (xx - 66) ** 2)


# ---- 3. lists, counts and minimum
@pytest.mark.parametrize('src_part,dst_part', [('boundary', 'boundary'), ('set', 'set'), ('set', 'clear')])
@pytest.mark.parametrize('n,h,w,s', [(9, 33, 65, 3), (3, 13, 70, 1), (2, 20, 130, 50), (1, 1, 70, 1)])
def test_lists_minimum_and_counts_equal_the_restatement(n, h, w, s, src_part, dst_part):
    st = blob_stack(n, h, w)
    want_lists, want_min, want_overlap = ref_lists(n, h, w, src_part, dst_part, s)
    d = dev(st)
    d2, off, tc, overlap = distance._lists_volume(d, d, PAIRS, src_part, dst_part, s, distance.DEFAULT_SCRATCH)
    assert off.shape == (len(PAIRS) + 1,) and tc.shape == (len(PAIRS),) and overlap.shape == (len(PAIRS), 3)
    assert lists_equal((d2, off, tc), want_lists) and np.array_equal(overlap, want_overlap)
    assert lists_equal(distance.directed_distances_volume(d, d, PAIRS, src_part, dst_part, s), want_lists)
    got_min = distance.pair_minimum_volume(d, d, PAIRS, src_part, dst_part, s)
    assert got_min.dtype == np.uint64 and got_min.shape == (len(PAIRS),) and np.array_equal(got_min, want_min)
    # an empty target is DIST_NONE for the whole volume, although other channels are populated; an empty query has no entry
    p = PAIRS.index((2, 3))
    if dst_part != 'clear':
        assert off[p + 1] > off[p] and (d2[off[p]:off[p + 1]] == distance.DIST_NONE).all() and int(got_min[p]) >> 32 == distance.DIST_NONE
    p = PAIRS.index((3, 2))
    assert off[p + 1] == off[p] and int(got_min[p]) == 2 ** 64 - 1
    # two stacks of different channel counts, one from a misaligned base
    a, b = misaligned(st[..., :4]), dev(st[..., 1:3])
    pairs = [(0, 0), (1, 1), (2, 0), (3, 1)]
    assert lists_equal(distance.directed_distances_volume(a, b, pairs, src_part, dst_part, s), R3.directed(st[..., :4], st[..., 1:3], pairs, src_part, dst_part, s))
    assert np.array_equal(distance.pair_minimum_volume(a, b, pairs, src_part, dst_part, s), R3.pair_min(st[..., :4], st[..., 1:3], pairs, src_part, dst_part, s))


def test_default_pairs_are_equal_channels():
    st = blob_stack(3, 13, 70)
    d = dev(st)
    assert lists_equal(distance.directed_distances_volume(d, d, slice_step=3), R3.directed(st, st, [(c, c) for c in range(5)], s=3))
    with pytest.raises(ValueError):
        distance.directed_distances_volume(d, d[..., :4].contiguous())
    with pytest.raises(ValueError):
        distance.directed_distances_volume(d, d, [(0, 5)])
    with pytest.raises(ValueError, match='must agree'):
        distance.directed_distances_volume(d, d[:2].contiguous())


def test_a_short_key_buffer_raises_and_nothing_is_stored_past_it():
    """The guard of the key store is what is under test: positions at or past the capacity are dropped on the device."""
    n, h, w, s = 9, 33, 65, 3
    d = dev(blob_stack(n, h, w))
    (want_d2, want_off, _), _, _ = ref_lists(n, h, w, 'boundary', 'boundary', s)
    total = int(want_off[-1])
    assert total > 100
    npairs, dims = len(PAIRS), (n, h, w, 5, 5)
    pairs_dev = torch.tensor(PAIRS, dtype=torch.int32, device='cuda')
    offsets = torch.from_numpy(want_off[:-1].copy()).cuda()
    guard = 64
    keys = torch.full((total + guard,), -7, dtype=torch.int64, device='cuda')
    distance._fill_keys_volume(d, d, pairs_dev, npairs, 2, 2, s, dims, offsets, keys, total, distance.DEFAULT_SCRATCH)
    assert (keys[total:] == -7).all()
    got = torch.sort(keys[:total]).values
    assert np.array_equal(host(got & 0xffffffff), want_d2)
    assert np.array_equal(np.bincount(host(got >> 32), minlength=npairs), np.diff(want_off))
    keys.fill_(-7)
    with pytest.raises(RuntimeError, match='key buffer'):
        distance._fill_keys_volume(d, d, pairs_dev, npairs, 2, 2, s, dims, offsets, keys, total - 1, distance.DEFAULT_SCRATCH)
    torch.cuda.synchronize()
    assert (keys[total - 1:] == -7).all()                               # the dropped key's slot and the guard tail are untouched
    assert int((keys[:total - 1] != -7).sum()) == total - 1
    keys.fill_(-7)                                                      # offsets that point past the buffer altogether
    with pytest.raises(RuntimeError, match='key buffer'):
        distance._fill_keys_volume(d, d, pairs_dev, npairs, 2, 2, s, dims, offsets + (1 << 40), keys, total, distance.DEFAULT_SCRATCH)
    torch.cuda.synchronize()
    assert (keys == -7).all()


# ---- 4. banding
def test_results_do_not_depend_on_the_banding():
    n, h, w, s = 9, 33, 65, 3
    st = blob_stack(n, h, w)
    d = dev(st)
    lib = L.lib()
    size = lambda rows, cb=0, pairs=0: int(lib.octseg_volume_distance_scratch_bytes(n, h, w, 5, cb, pairs, rows))
    assert distance.volume_bands(n, h, w, 5)[:2] == (h, 1)               # the default budget takes the frame at once
    whole = {p: distance.distance_volume(d, to=p, slice_step=s) for p in PARTS}
    for rows in (8, 5, 1):                                               # 5, 7 and 33 bands; 33 = 4 * 8 + 1: a last band of one row
        budget = size(rows) + 3
        assert distance.volume_bands(n, h, w, 5, scratch_bytes=budget) == (rows, -(-h // rows), size(rows)) and -(-h // rows) >= 3
        for p in PARTS:
            assert torch.equal(distance.distance_volume(d, to=p, slice_step=s, scratch_bytes=budget), whole[p]), (rows, p)
    assert np.array_equal(host(whole['boundary']), ref_maps(n, h, w, s)['boundary'])
    npairs = len(PAIRS)
    whole_lists = distance._lists_volume(d, d, PAIRS, 'boundary', 'boundary', s, distance.DEFAULT_SCRATCH)
    whole_min = distance.pair_minimum_volume(d, d, PAIRS, slice_step=s)
    for rows in (10, 4, 1):
        budget = size(rows, 5, npairs)
        assert distance.volume_bands(n, h, w, 5, 5, npairs, budget)[:2] == (rows, -(-h // rows)) and -(-h // rows) >= 3
        got = distance._lists_volume(d, d, PAIRS, 'boundary', 'boundary', s, budget)
        assert all(np.array_equal(a, b) for a, b in zip(got, whole_lists))
        assert np.array_equal(distance.pair_minimum_volume(d, d, PAIRS, slice_step=s, scratch_bytes=budget), whole_min)
    assert lists_equal(whole_lists[:3], ref_lists(n, h, w, 'boundary', 'boundary', s)[0])
    # a budget below the smallest band raises and names the bytes needed, from the wrapper and from the library
    for fn, need in ((lambda b: distance.distance_volume(d, slice_step=s, scratch_bytes=b), size(1)),
                     (lambda b: distance.directed_distances_volume(d, d, PAIRS, slice_step=s, scratch_bytes=b), size(1, 5, npairs)),
                     (lambda b: distance.pair_minimum_volume(d, d, PAIRS, slice_step=s, scratch_bytes=b), size(1, 5, npairs))):
        with pytest.raises(ValueError, match=str(need)):
            fn(need - 1)
    scratch = torch.empty((size(1),), dtype=torch.uint8, device='cuda')
    out = torch.full((n, 5, h, w), -7, dtype=torch.int32, device='cuda')
    assert lib.octseg_volume_distance(L.ptr(d), n, h, w, 5, 0, s, L.ptr(scratch), size(1) - 1, L.ptr(out), None) == -5
    assert str(size(1)).encode() in lib.octseg_last_error()
    torch.cuda.synchronize()
    assert (out == -7).all()


# ---- 5. the report
@functools.lru_cache(maxsize=None)
def golden():
    """Slices 27 .. 32 of the fixture, rows 420 .. 599 and columns 220 .. 399: lumen everywhere, cap and lipid core on 28 .. 30, vasa vasorum on
    30 .. 32; the prediction is the same volume rolled by one slice and by (3, 5) pixels."""
    truth = load_fixture(FIXTURE)['stack'][27:33, 420:600, 220:400].astype(np.float32)
    pred = np.roll(truth, (1, 3, 5), axis=(0, 1, 2))
    truth.setflags(write=False)
    pred.setflags(write=False)
    return pred, truth


@functools.lru_cache(maxsize=None)
def golden_ref(s):
    pred, truth = golden()
    pairs = [(c, c) for c in range(4)]
    return (R3.directed(pred, truth, pairs, s=s), R3.directed(truth, pred, pairs, s=s), R3.overlap(pred, truth, pairs),
            R3.pair_min(truth, truth, [(2, 0)], 'set', 'set', s))


def test_golden_volume_surface_metrics_and_cap_distance():
    pred, truth = golden()
    assert all(truth[..., c].any() for c in range(4))
    s = 4
    ab, ba, overlap, want_min = golden_ref(s)
    dp, dt = dev(pred), dev(truth)
    d2, offsets, counts = distance._volume_surface_lists(dp, dt, [(c, c) for c in range(4)], s)
    assert lists_equal((d2[0], offsets[0], ab[2]), ab) and lists_equal((d2[1], offsets[1], ba[2]), ba) and np.array_equal(counts, overlap)
    got = distance.volume_surface_metrics(dp, dt, slice_step=s)
    names = ['Lumen', 'Fibrous cap', 'Lipid core', 'Vasa vasorum']
    assert got == distance.build_volume_surface_metrics((ab[0], ba[0]), (ab[1], ba[1]), overlap, names)          # float64 equality
    assert list(got) == names
    for col in got.values():
        assert col['hd'] is not None and 0 < col['assd'] <= col['hd'] and 0 <= col['hd95'] <= col['hd'] and 0 < col['dice'] < 1
    quarter = distance.volume_surface_metrics(dp, dt, slice_step=s, ratio=4)
    assert quarter['Lumen']['hd'] == got['Lumen']['hd'] / 4 and quarter['Lumen']['dice'] == got['Lumen']['dice']
    assert np.array_equal(distance.pair_minimum_volume(dt, dt, [(2, 0)], 'set', 'set', s), want_min)
    cap = distance.cap_distance_volume(dt, slice_step=s)
    assert cap == distance.build_cap_distance_volume(want_min[0], 180, 180)
    z, y, x = cap['at']
    assert truth[z, y, x, 2] and cap['distance'] == float(np.sqrt(np.float64(cap['d2'])))
    flat = distance.cap_distance(dt)                                      # the per-slice minimum bounds the volume's from above
    assert cap['d2'] <= min(flat['d2'])
    named = distance.cap_distance_volume(dt, classes=names, slice_step=s, ratio=112)
    assert named == distance.build_cap_distance_volume(want_min[0], 180, 180, ratio=112) and named['d2'] == cap['d2'] and named['at'] == cap['at']
    assert named['distance'] < cap['distance'] / 100
    assert distance.cap_distance_volume(dt, lumen='Vasa vasorum', lipid='Lumen', slice_step=s) is not None
    empty = torch.zeros_like(dt)
    empty[..., 0] = dt[..., 0]
    assert distance.cap_distance_volume(empty) is None                    # no lipid core anywhere in the volume
    with pytest.raises(ValueError):
        distance.cap_distance_volume(dt[..., :2].contiguous())


def test_the_cap_can_be_thinner_across_slices_than_inside_any():
    st = np.zeros((2, 24, 40, 4), np.float32)
    st[0, 5, 5, 0] = st[1, 20, 30, 0] = 1                                # lumen
    st[0, 5, 30, 2] = st[1, 5, 6, 2] = 1                                 # lipid core: 25 away inside slice 0, further inside slice 1
    d = dev(st)
    flat = distance.cap_distance(d)
    assert flat['slice'] == [0, 1] and flat['d2'] == [625, 15 ** 2 + 24 ** 2]
    cap = distance.cap_distance_volume(d, slice_step=1)
    assert cap == {'distance': float(np.sqrt(np.float64(2))), 'at': (1, 5, 6), 'd2': 2}
    assert cap['distance'] < min(flat['distance'])
    assert distance.cap_distance_volume(d, slice_step=30) == {'distance': 25.0, 'at': (0, 5, 30), 'd2': 625}


def test_command_line_round_trip(tmp_path):
    from PIL import Image
    pred_dir, truth_dir = tmp_path / 'pred', tmp_path / 'truth'
    pred_dir.mkdir()
    truth_dir.mkdir()
    n, h, w = 3, 20, 40
    vol = {'pred': np.stack([R3.blob_volume(n, h, w, 10 + c, size=0.6) for c in range(4)], axis=-1),
           'truth': np.stack([R3.blob_volume(n, h, w, 20 + c, size=0.6) for c in range(4)], axis=-1)}
    for folder, name in ((pred_dir, 'pred'), (truth_dir, 'truth')):
        for z in range(n):
            Image.fromarray((vol[name][z] * 255).astype(np.uint8)).save(str(folder / f's{z}.tiff'))
    plain, stepped = tmp_path / 'plain', tmp_path / 'stepped'
    distance.main([str(pred_dir), str(truth_dir), str(plain)])
    distance.main([str(pred_dir), str(truth_dir), str(stepped), 'slice_step=4'])
    assert sorted(os.listdir(plain)) == ['surface_metrics.json']          # the new file is written only with slice_step=
    assert sorted(os.listdir(stepped)) == ['surface_metrics.json', 'surface_metrics_3d.json']
    assert open(plain / 'surface_metrics.json').read() == open(stepped / 'surface_metrics.json').read()
    saved = json.load(open(stepped / 'surface_metrics_3d.json'))
    names = ['Lumen', 'Fibrous cap', 'Lipid core', 'Vasa vasorum']
    assert saved['images'] == ['s0.tiff', 's1.tiff', 's2.tiff'] and saved['slice_step'] == 4 and saved['unit'] == 'pixel' and saved['classes'] == names
    pairs = [(c, c) for c in range(4)]
    ab, ba = R3.directed(vol['pred'], vol['truth'], pairs, s=4), R3.directed(vol['truth'], vol['pred'], pairs, s=4)
    want = distance.build_volume_surface_metrics((ab[0], ba[0]), (ab[1], ba[1]), R3.overlap(vol['pred'], vol['truth'], pairs), names)
    assert saved['metrics'] == json.loads(json.dumps(want))


def test_wrappers_refuse_wrong_dtype_rank_extents_and_step():
    ok = torch.zeros((3, 4, 4, 4), device='cuda')
    calls = (distance.boundary_volume, distance.distance_volume, lambda s: distance.directed_distances_volume(s, s), distance.cap_distance_volume,
             lambda s: distance.volume_surface_metrics(s, s))
    for bad in (ok.double(), ok[0], torch.zeros((1, 0, 4, 4), device='cuda'), torch.zeros((1, 4, 4, 17), device='cuda'),
                torch.zeros((1, 1, 4097, 1), device='cuda')):
        for fn in calls:
            with pytest.raises(ValueError):
                fn(bad)
    for fn in (lambda s: distance.distance_volume(ok, slice_step=s), lambda s: distance.directed_distances_volume(ok, ok, slice_step=s),
               lambda s: distance.cap_distance_volume(ok, slice_step=s), lambda s: distance.volume_surface_metrics(ok, ok, slice_step=s)):
        for bad in (0, 1.5, 16384):                                      # 16384 * 2 > 32767
            with pytest.raises(ValueError):
                fn(bad)
        fn(16383)
