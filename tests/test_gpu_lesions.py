"""Lesions in 3-D on the GPU (csrc/lesions.hip through oct_segmentation_amd/lesions.py) against the scipy reference of tests/lesions_ref.py.
Every comparison is integer equality: there is no tolerance in this feature."""
import functools
import json
import os

import numpy as np
import pytest
import torch
from PIL import Image

import lesions_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import analysis, cleanup, lesions
from oct_segmentation_amd.model import CLASS_IDS

pytestmark = pytest.mark.gpu

ACROSS = ['overlap', 'full']
SHAPES = [(1, 1), (4, 5), (37, 63), (5, 64), (9, 65), (97, 130)]       # below, at and above one 64-pixel word; more than one block
DENSITY = [0.45, 0.03, 0.25, 0.9, 0.12]


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()        # a copy: the cached stacks are read-only


def host(t):
    return t.cpu().numpy()


def vol_stack(*vols):
    """[N, H, W, len(vols)] from 3-D volumes."""
    return np.stack([np.asarray(v, np.float32) for v in vols], axis=-1)


@functools.lru_cache(maxsize=None)
def seeded_stack(n, h, w, c):
    """[n, h, w, c]: channel i random at DENSITY[i].  Read-only: shared between tests."""
    rng = np.random.RandomState(100000 * n + 1000 * h + 10 * w + c)
    st = np.stack([rng.rand(n, h, w) < DENSITY[i] for i in range(c)], axis=-1).astype(np.float32)
    st.setflags(write=False)
    return st


def check_all(st, across, d=None):
    """Labels, table and profile of a stack equal the reference's; returns the reference's (nles, top, profile)."""
    d = dev(st) if d is None else d
    n, h, w, c = st.shape
    ref = [R.analyse(st[..., i], across) for i in range(c)]
    labels = lesions.label_volume(d, across=across)
    assert labels.dtype == torch.int32 and tuple(labels.shape) == (c, n, h, w)
    assert np.array_equal(host(labels), np.stack([r[0] for r in ref]))
    nles, top, prof = lesions.lesion_table(d, across=across, profile=True)
    assert nles.dtype == top.dtype == prof.dtype == torch.int32
    assert tuple(nles.shape) == (c,) and tuple(top.shape) == (c, 32, 8) and tuple(prof.shape) == (c, 32, n)
    want = (np.array([r[1] for r in ref], np.int32), np.stack([r[2] for r in ref]), np.stack([r[3] for r in ref]))
    assert np.array_equal(host(nles), want[0]) and np.array_equal(host(top), want[1]) and np.array_equal(host(prof), want[2])
    n2, top2 = lesions.lesion_table(d, across=across)
    assert torch.equal(n2, nles) and torch.equal(top2, top)
    return want


# ---- 1. random blobs
@pytest.mark.parametrize('across', ACROSS)
@pytest.mark.parametrize('h,w', SHAPES)
def test_random_blobs_equal_the_reference(h, w, across):
    for n in (1, 2, 3, 5):
        for c in (1, 4, 5):
            st = seeded_stack(n, h, w, c)
            d = dev(st)
            check_all(st, across, d)
            if n == 1:                                                  # one slice: the 2-D labelling, channel-major instead of slice-major
                assert torch.equal(lesions.label_volume(d, across=across), cleanup.label_stack(d).permute(1, 0, 2, 3))


# ---- 2. designed volumes
def staircase_x(n, h, w):
    """One pixel moving +1 in x per slice across the x = 63 / 64 seam."""
    v = np.zeros((n, h, w), bool)
    for z in range(n):
        v[z, h // 2, 64 - n // 2 + z] = True
    return v


def staircase_y(n, h, w):
    v = np.zeros((n, h, w), bool)
    for z in range(n):
        v[z, 1 + z, 63 + (z % 2)] = True                                # moving in y, hopping over the seam as well
    return v


def late_join(n, h, w):
    """Two columns, separate in slices 0 .. n - 2, that join in the last slice only."""
    v = np.zeros((n, h, w), bool)
    v[:, 2:h - 2, 3] = True
    v[:, 2:h - 2, w - 4] = True
    v[n - 1, h - 3, 3:w - 3] = True
    return v


def checker3(n, h, w):
    zz, yy, xx = np.mgrid[:n, :h, :w]
    return (zz + yy + xx) % 2 == 0


def full(n, h, w):
    return np.ones((n, h, w), bool)


def empty(n, h, w):
    return np.zeros((n, h, w), bool)


def last_voxel(n, h, w):
    v = np.zeros((n, h, w), bool)
    v[-1, -1, -1] = True
    return v


def every_second(n, h, w):
    v = np.zeros((n, h, w), bool)
    v[::2, 3:9, 60:70] = True
    return v


DESIGNED = {'staircase_x': staircase_x, 'staircase_y': staircase_y, 'late_join': late_join, 'checker3': checker3, 'full': full, 'empty': empty,
            'last_voxel': last_voxel, 'every_second': every_second}


@pytest.mark.parametrize('transposed', [False, True])
@pytest.mark.parametrize('name', sorted(DESIGNED))
def test_designed_volumes(name, transposed):
    n, h, w = 6, 12, 130
    v = DESIGNED[name](n, h, w)
    if transposed:
        v = np.ascontiguousarray(v.transpose(0, 2, 1))
        h, w = w, h
    st = vol_stack(v)
    for across in ACROSS:
        nles, top, prof = check_all(st, across)
        count = int(nles[0])
        if name.startswith('staircase') or name == 'checker3':
            assert count == (1 if across == 'full' else n)             # diagonal contact across slices is contact under `full` only
        if name == 'late_join':
            assert count == 1 and top[0, 0, 1] == v.reshape(-1).argmax() < h * w and top[0, 0, 2] == 0     # the smallest index, in slice 0
            two = check_all(st[:n - 1], across)
            assert int(two[0][0]) == 2
        if name == 'full':
            assert count == 1 and top[0, 0].tolist() == [n * h * w, 0, 0, n - 1, 0, h - 1, 0, w - 1]
        if name == 'empty':
            assert count == 0 and not top.any() and not prof.any()
        if name == 'last_voxel':
            assert top[0, 0].tolist() == [1, n * h * w - 1, n - 1, n - 1, h - 1, h - 1, w - 1, w - 1]
        if name == 'every_second':
            assert count == 3 and (top[0, :3, 2] == top[0, :3, 3]).all()
            assert not host(lesions.clean_volume(dev(st), min_slices=2, across=across)).any()       # every lesion is one slice long


# ---- 3. the flicker filter, keep and min_voxels
def flicker_volume():
    """[5, 40, 100]: a persistent blob in every slice, a speck alone in slice 2, a speck in slice 3 that overlaps a blob of slice 4."""
    v = np.zeros((5, 40, 100), bool)
    v[:, 5:15, 58:70] = True
    v[2, 30, 80] = True                                                  # flicker
    v[4, 30:32, 20:23] = True
    v[3, 31, 22] = True
    return v


@pytest.mark.parametrize('across', ACROSS)
def test_flicker_filter_removes_exactly_the_lone_speck(across):
    v = flicker_volume()
    st = vol_stack(v, v[::-1], np.zeros_like(v), np.ones_like(v))
    d = dev(st)
    before = d.clone()
    got = lesions.clean_volume(d, across=across)                         # min_slices = 2 is the default
    assert got.dtype == torch.float32 and got.shape == d.shape
    assert np.array_equal(host(got), R.clean_stack(st, 2, 0, 0, across))
    want = v.copy()
    want[2, 30, 80] = False
    assert np.array_equal(host(got)[..., 0], want) and int(v.sum()) - int(want.sum()) == 1
    assert torch.equal(d, before)                                        # the input is not written
    for kw in (dict(min_slices=1), dict(min_slices=3), dict(min_slices=5), dict(min_slices=6), dict(min_slices=1, min_voxels=2),
               dict(min_slices=1, keep=1), dict(min_slices=1, keep=2), dict(min_slices=2, keep=3, min_voxels=7), dict(min_slices=1, keep=40)):
        out, (nles, top) = lesions.clean_volume(d, across=across, return_table=True, **kw)
        want = R.clean_stack(st, kw.get('min_slices'), kw.get('min_voxels', 0), kw.get('keep', 0), across)
        assert np.array_equal(host(out), want), kw
        wn, wt, _ = R.table_stack(want, across)                          # the table describes the kept lesions
        assert np.array_equal(host(nles), wn) and np.array_equal(host(top), wt), kw


def test_keep_with_a_four_way_tie_at_the_threshold():
    v = np.zeros((3, 40, 100), bool)
    v[:, 2:12, 2:12] = True
    for x in (20, 40, 62, 80):
        v[0:2, 20:23, x:x + 3] = True                                    # four lesions of 18 voxels
    v[1, 35, 50] = True
    st = vol_stack(v)
    assert [r[0] for r in R.lesions(v)] == [300, 18, 18, 18, 18, 1]
    for keep in (1, 2, 3, 5, 6, 7):
        out, (nles, top) = lesions.clean_volume(dev(st), min_slices=1, keep=keep, return_table=True)
        want = R.clean_stack(st, 1, 0, keep)
        assert np.array_equal(host(out), want), keep
        assert int(nles[0]) == (1 if keep == 1 else 5 if keep <= 5 else 6)         # the largest and all four of the tie; the speck only from 6 on
        assert np.array_equal(host(top), R.table_stack(want)[1])


# ---- 4. table limits
def test_thirty_four_equal_lesions_rank_by_first_voxel_and_truncate():
    n, h, w = 2, 24, 140
    v = np.zeros((n, h, w), bool)
    spots = [(z, y + 3 * z, x) for z in range(n) for y in (1, 7, 13, 19) for x in (2, 40, 62, 100, 130)][:34]     # slice 1 sits between slice 0's rows
    for z, y, x in spots:
        v[z, y:y + 2, x:x + 3] = True                                    # 34 lesions of 6 voxels, no two in contact
    st = vol_stack(v)
    for across in ACROSS:
        nles, top, prof = check_all(st, across)
        assert int(nles[0]) == 34 and (top[0, :, 0] == 6).all()
        firsts = sorted(z * h * w + y * w + x for z, y, x in spots)
        assert top[0, :, 1].tolist() == firsts[:32]                     # rows 32 and 33 of the ranking are the two that are not listed
        rep = lesions.lesion_report(dev(st), across=across, classes=['c'])
        assert rep['c']['n_lesions'] == 34 and rep['c']['truncated'] is True and len(rep['c']['lesions']) == 32


# ---- 5. the demo excerpt
@pytest.mark.parametrize('across', ACROSS)
def test_golden_excerpt(across):
    stack, names, recorded = R.golden_stack()
    d = torch.from_numpy(np.array(stack)).cuda().to(torch.float32)
    nles, top, prof = lesions.lesion_table(d, across=across, profile=True)
    labels = lesions.label_volume(d, across=across)
    want_n = {'overlap': [1, 5, 5, 17], 'full': [1, 5, 5, 16]}[across]
    out, (n2, top2) = lesions.clean_volume(d, min_slices=2, across=across, return_table=True)
    assert host(n2).tolist() == {'overlap': [1, 4, 4, 8], 'full': [1, 4, 4, 7]}[across]
    for c in range(4):
        lab, n, t, p = R.analyse(stack[..., c], across)
        assert n == want_n[c] <= 32
        assert torch.equal(labels[c], torch.from_numpy(lab).cuda()), c
        assert int(nles[c]) == n and np.array_equal(host(top[c]), t) and np.array_equal(host(prof[c]), p), c
        # the flicker filter, from the same labelling (all lesions are listed: n <= 32): the rows that span two slices or more, and their voxels
        rows = t[:n][t[:n, 3] - t[:n, 2] + 1 >= 2]
        assert int(n2[c]) == len(rows) and np.array_equal(host(top2[c, :len(rows)]), rows) and not top2[c, len(rows):].any(), c
        want = np.isin(lab, rows[:, 1] + 1)
        assert torch.equal(out[..., c], torch.from_numpy(want).cuda().to(torch.float32)), c
    counts = analysis.measure_stack(d)[0]                                # [N, channels]
    assert torch.equal(prof.sum(dim=1).T.contiguous().to(torch.int32), counts)      # valid because nles <= 32: every set pixel is in a ranked lesion
    rep = lesions.lesion_report(d, names, ratio=recorded['ratio'], across=across)
    assert rep == lesions.build_report(host(nles), host(top), host(prof), 750, 750, image_names=names, ratio=recorded['ratio'])
    assert rep['Lumen']['lesions'][0]['area_ratio'] == recorded['objects']['Lumen']['area']
    assert lesions.lesion_report(d, names, across=across, clean=True) == lesions.lesion_report(out, names, across=across)


# ---- 6. chunking
def test_channel_by_channel_equals_all_channels():
    n, h, w, c = 3, 37, 63, 5
    st = seeded_stack(n, h, w, c)
    d = dev(st)
    lib = L.lib()
    one, every = int(lib.octseg_lesions_scratch_bytes(1, n, h, w)), int(lib.octseg_lesions_scratch_bytes(c, n, h, w))
    assert one < every
    for across in ACROSS:
        labels = lesions.label_volume(d, across=across)
        table = lesions.lesion_table(d, across=across, profile=True)
        out, kept = lesions.clean_volume(d, min_slices=2, keep=20, across=across, return_table=True)
        for budget in (one, every - 1):
            assert torch.equal(lesions.label_volume(d, across=across, scratch_bytes=budget), labels)
            for a, b in zip(lesions.lesion_table(d, across=across, profile=True, scratch_bytes=budget), table):
                assert torch.equal(a, b)
            o2, k2 = lesions.clean_volume(d, min_slices=2, keep=20, across=across, return_table=True, scratch_bytes=budget)
            assert torch.equal(o2, out) and torch.equal(k2[0], kept[0]) and torch.equal(k2[1], kept[1])
    with pytest.raises(ValueError, match=str(one)):                      # not even one channel fits: the need is named
        lesions.label_volume(d, scratch_bytes=one - 1)


# ---- 7. guard bands
def test_outputs_stay_inside_their_extent_and_refused_calls_launch_nothing():
    n, h, w, c = 3, 9, 65, 4
    st = seeded_stack(n, h, w, c)
    d = dev(st)
    before = d.clone()
    lib = L.lib()
    need = int(lib.octseg_lesions_scratch_bytes(c, n, h, w))
    scratch = torch.empty((need,), dtype=torch.uint8, device='cuda')
    labels = torch.full((c + 1, n, h, w), 7, dtype=torch.int32, device='cuda')
    nles = torch.full((c + 1,), 7, dtype=torch.int32, device='cuda')
    top = torch.full((c + 1, 32, 8), 7, dtype=torch.int32, device='cuda')
    prof = torch.full((c + 1, 32, n), 7, dtype=torch.int32, device='cuda')
    out = torch.full((n + 1, h, w, c), 7.0, dtype=torch.float32, device='cuda')
    s = L.stream_ptr()

    def comp(stack=L.ptr(d), nn=n, hh=h, ch=c, across=0, scr=L.ptr(scratch), nbytes=need, lab=L.ptr(labels)):
        return lib.octseg_volume_components(stack, nn, hh, w, ch, across, scr, nbytes, lab, L.ptr(nles), L.ptr(top), L.ptr(prof), s)

    def clean(ch=c, across=0, keep=0, min_voxels=0, min_slices=2, nbytes=need, dst=L.ptr(out)):
        return lib.octseg_volume_cleanup(L.ptr(d), n, h, w, ch, across, keep, min_voxels, min_slices, L.ptr(scratch), nbytes, dst, L.ptr(nles),
                                         L.ptr(top), s)

    # refused calls first: nothing may be written
    assert comp(scr=None) == -5 and comp(nbytes=need - 1) == -5 and comp(across=2) == -5 and comp(stack=None) == -5
    assert comp(hh=0) == -1 and comp(ch=17) == -1 and comp(nn=0) == -1
    assert clean(ch=17) == -1 and clean(across=3) == -5 and clean(keep=-1) == -5 and clean(min_voxels=-1) == -5 and clean(min_slices=0) == -5
    assert clean(nbytes=need - 1) == -5 and clean(dst=None) == -5 and clean(dst=L.ptr(d)) == -5
    torch.cuda.synchronize()
    assert (labels == 7).all() and (nles == 7).all() and (top == 7).all() and (prof == 7).all() and (out == 7).all()
    for across in (0, 1):
        name = ACROSS[across]
        L.check(comp(across=across))
        assert np.array_equal(host(labels[:c]), R.label_stack(st, name))
        wn, wt, wp = R.table_stack(st, name)
        assert np.array_equal(host(nles[:c]), wn) and np.array_equal(host(top[:c]), wt) and np.array_equal(host(prof[:c]), wp)
        assert (labels[c] == 7).all() and (nles[c] == 7).all() and (top[c] == 7).all() and (prof[c] == 7).all()
        L.check(clean(across=across, keep=9, min_voxels=2))
        want = R.clean_stack(st, 2, 2, 9, name)
        assert np.array_equal(host(out[:n]), want) and (out[n] == 7).all() and (nles[c] == 7).all() and (top[c] == 7).all()
        assert np.array_equal(host(nles[:c]), R.table_stack(want, name)[0]) and np.array_equal(host(top[:c]), R.table_stack(want, name)[1])
    assert torch.equal(d, before)                                        # the input stack is never modified


# ---- 7b. the scratch is work space only: no result depends on what it held (the labelling initialises its counters at run starts only)
SCRATCH_FILLS = (0x00, 0xFF, 0x55)


def _same_for_every_fill(got, want, names, what):
    for fill, g in zip(SCRATCH_FILLS, got):
        for name, a, b, first in zip(names, g, want, got[0]):
            assert np.array_equal(a, first), f'{what}: {name} differs between scratch fills 0x00 and {fill:#04x}'
            assert np.array_equal(a, b), f'{what}: {name} differs from the reference with scratch fill {fill:#04x}'


@pytest.mark.parametrize('across', [0, 1])
def test_volume_calls_do_not_depend_on_the_scratch(across):
    n, h, w, c = 3, 9, 65, 3
    st = seeded_stack(n, h, w, c)
    d = dev(st)
    lib = L.lib()
    need = int(lib.octseg_lesions_scratch_bytes(c, n, h, w))
    s = L.stream_ptr()
    comps, cleans = [], []
    for fill in SCRATCH_FILLS:
        labels = torch.full((c, n, h, w), 7, dtype=torch.int32, device='cuda')
        nles = torch.full((c,), 7, dtype=torch.int32, device='cuda')
        top = torch.full((c, 32, 8), 7, dtype=torch.int32, device='cuda')
        prof = torch.full((c, 32, n), 7, dtype=torch.int32, device='cuda')
        out = torch.full((n, h, w, c), 7.0, dtype=torch.float32, device='cuda')
        scratch = torch.full((need,), fill, dtype=torch.uint8, device='cuda')
        L.check(lib.octseg_volume_components(L.ptr(d), n, h, w, c, across, L.ptr(scratch), need, L.ptr(labels), L.ptr(nles), L.ptr(top), L.ptr(prof), s))
        comps.append((host(labels), host(nles), host(top), host(prof)))
        scratch.fill_(fill)
        L.check(lib.octseg_volume_cleanup(L.ptr(d), n, h, w, c, across, 2, 0, 2, L.ptr(scratch), need, L.ptr(out), L.ptr(nles), L.ptr(top), s))
        cleans.append((host(out), host(nles), host(top)))
    name = ACROSS[across]
    _same_for_every_fill(comps, (R.label_stack(st, name),) + tuple(R.table_stack(st, name)), ('labels', 'nles', 'top', 'profile'), 'volume_components')
    kept = R.clean_stack(st, 2, 0, 2, name)
    _same_for_every_fill(cleans, (kept,) + tuple(R.table_stack(kept, name)[:2]), ('out', 'nles', 'top'), 'volume_cleanup')


def test_wrappers_refuse_wrong_dtype_rank_and_channels():
    for bad in (torch.zeros((2, 4, 4, 4), dtype=torch.float64, device='cuda'), torch.zeros((4, 4, 4), device='cuda'),
                torch.zeros((2, 0, 4, 4), device='cuda'), torch.zeros((2, 4, 4, 17), device='cuda')):
        for fn in (lesions.label_volume, lesions.lesion_table, lesions.clean_volume, lesions.lesion_report):
            with pytest.raises(ValueError):
                fn(bad)
    ok = torch.zeros((2, 4, 4, 4), device='cuda')
    with pytest.raises(ValueError, match='across'):
        lesions.label_volume(ok, across='6')
    with pytest.raises(ValueError, match='min_slices'):
        lesions.clean_volume(ok, min_slices=0)


# ---- 8. the command line
def _models_dir(cuda, root):
    from oct_segmentation_amd.model import OCTSegmentationModel
    specs = {'LM': ('unet', ['Lumen'], 64), 'FC_LC': ('linknet', ['Lipid core', 'Fibrous cap'], 96), 'VV': ('unet', ['Vasa vasorum'], 64)}
    for d, (arch, classes, size) in specs.items():
        os.makedirs(os.path.join(root, d))
        m = OCTSegmentationModel(arch, 'resnet18', f'{arch}_resnet18', 3, classes, device=cuda, seed=len(d) + 3, compute_dtype=torch.float32)
        m.save_checkpoint(os.path.join(root, d, 'weights.ckpt'))
        with open(os.path.join(root, d, 'config.json'), 'w') as f:
            json.dump({'model_name': f'{arch}_resnet18', 'architecture': arch, 'encoder': 'resnet18', 'input_size': size, 'classes': classes}, f)
    return root


def _files(d):
    out = {}
    for name in sorted(os.listdir(d)):
        with open(os.path.join(d, name), 'rb') as f:
            out[name] = f.read()
    return out


def test_predict_main_writes_lesions_json(cuda, tmp_path):
    """Both input kinds: a directory of files (sorted file-name order) and a .npy volume (analyze_pullback's stack)."""
    from oct_segmentation_amd import predict, pullback
    models = _models_dir(cuda, os.path.join(tmp_path, 'models'))
    rng = np.random.default_rng(23)
    data_dir = os.path.join(tmp_path, 'input')
    os.makedirs(data_dir)
    created = ['z_last', 'a_first', 'm_mid']                             # sorted order differs from creation order
    for name in created:
        Image.fromarray(rng.integers(0, 255, (90, 90, 3), dtype=np.uint8)).save(os.path.join(data_dir, f'{name}.png'))
    args = [f'data_dir={data_dir}', f'models_dir={models}', 'output_size=[120,120]', 'compute_dtype=fp32']
    off, on = os.path.join(tmp_path, 'off'), os.path.join(tmp_path, 'on')
    assert predict.main(args + [f'save_dir={off}']) == 0
    assert predict.main(args + [f'save_dir={on}', 'lesions=true']) == 0
    a, b = _files(off), _files(on)
    assert sorted(b) == sorted(list(a) + ['lesions.json'])
    for name in a:                                                       # overlays and colour masks do not change
        assert a[name] == b[name], name
    names = sorted(created)
    images, _ = predict.data_processing([os.path.join(data_dir, f'{n}.png') for n in names], [120, 120])
    stack = predict.segment_stack(images, [120, 120], list(CLASS_IDS), models, device='cuda', compute_dtype=torch.float32, device_preprocess=True)
    got = json.loads(b['lesions.json'])
    assert got == json.loads(json.dumps(lesions.lesion_report(stack, names)))
    assert any(v['n_lesions'] for v in got.values())                     # the nets found something to report
    cleaned = os.path.join(tmp_path, 'cleaned')
    assert predict.main(args + [f'save_dir={cleaned}', 'lesions=true', 'clean=true']) == 0
    assert json.loads(_files(cleaned)['lesions.json']) == json.loads(json.dumps(lesions.lesion_report(cleanup.clean_stack(stack), names)))
    # the volume path
    vol = rng.integers(0, 256, (2, 90, 90, 3), dtype=np.uint8)
    np.save(os.path.join(tmp_path, 'pull.npy'), vol)
    vargs = [f'data_dir={os.path.join(tmp_path, "pull.npy")}', f'models_dir={models}', 'output_size=[120,120]', 'compute_dtype=fp32']
    voff, von = os.path.join(tmp_path, 'voff'), os.path.join(tmp_path, 'von')
    assert predict.main(vargs + [f'save_dir={voff}']) == 0
    assert predict.main(vargs + [f'save_dir={von}', 'lesions=true']) == 0
    a, b = _files(voff), _files(von)
    assert sorted(b) == sorted(list(a) + ['lesions.json'])
    for name in a:
        assert a[name] == b[name], name
    res = pullback.analyze_pullback(vol, models, list(CLASS_IDS), output_size=(120, 120), names=['pull_001', 'pull_002'], compute_dtype=torch.float32)
    assert json.loads(b['lesions.json']) == json.loads(json.dumps(lesions.lesion_report(res.stack, ['pull_001', 'pull_002'])))
