"""Lesion matching on the GPU (csrc/match.hip through oct_segmentation_amd/match.py) against the restatement of tests/match_ref.py, which
tests/test_match.py proves against sklearn's contingency matrix on the same cases.  Every comparison is integer equality: there is no tolerance in
this feature."""
import json

import numpy as np
import pytest
import torch
from PIL import Image

import match_ref as R
from oct_segmentation_amd import _lib as L
from oct_segmentation_amd import distance, lesions, match

pytestmark = pytest.mark.gpu

ACROSS = ['overlap', 'full']
NAMES = ('nles', 'top', 'overlap', 'frames')


def dev(a):
    return torch.from_numpy(np.array(a, dtype=np.float32)).cuda()        # a copy: the cached stacks are read-only


def host(t):
    return t.cpu().numpy()


def assert_equal_tables(got, want, what=''):
    for name, a, b in zip(NAMES, got, want):
        a = host(a) if torch.is_tensor(a) else a
        assert a.dtype == np.int32 and a.shape == b.shape, (what, name, a.shape, b.shape)
        assert np.array_equal(a, b), f'{what}: {name} differs from the restatement'


# ---- 1. every case, both rules, all four outputs
@pytest.mark.parametrize('across', ACROSS)
@pytest.mark.parametrize('name', sorted(R.CASES))
def test_all_four_outputs_equal_the_restatement(name, across):
    pred, truth = R.case(name)
    n, h, w, c = pred.shape
    dp, dt = dev(pred), dev(truth)
    before = dp.clone(), dt.clone()
    m = match.match_volumes(dp, dt, across=across)
    assert all(t.dtype == torch.int32 and t.is_cuda for t in m)
    assert tuple(m.nles.shape) == (c, 2) and tuple(m.top.shape) == (c, 2, 32, 8) and tuple(m.overlap.shape) == (c, 33, 33)
    assert tuple(m.frames.shape) == (c, n, 3)
    assert_equal_tables(m, R.case_tables(name, across), f'{name} {across}')
    assert torch.equal(dp, before[0]) and torch.equal(dt, before[1])     # neither stack is written
    again = match.match_volumes(dp, dt, across=across)                   # two runs are bit-equal
    assert all(torch.equal(a, b) for a, b in zip(m, again))
    bare = match.match_volumes(dp, dt, across=across, want_top=False, want_frames=False)
    assert bare.top is None and bare.frames is None and torch.equal(bare.nles, m.nles) and torch.equal(bare.overlap, m.overlap)
    # top equals two lesion_table calls; frames equals the boundary-distance call's overlap counts
    for side, d in enumerate((dp, dt)):
        nles, top = lesions.lesion_table(d, across=across)
        assert torch.equal(m.nles[:, side], nles) and torch.equal(m.top[:, side], top)
    counts = distance._lists(dp, dt, None, 'set', 'set', distance.DEFAULT_SCRATCH)[3]      # [N, channels, 3]
    assert np.array_equal(host(m.frames), counts.transpose(1, 0, 2))


def test_designed_pairs_say_what_they_were_designed_to():
    same = match.match_volumes(*(dev(v) for v in R.case('same')))
    for c in range(2):
        vox = host(same.top[c, 0, :, 0])
        assert np.array_equal(host(same.overlap[c]), np.diag(np.concatenate([vox, [0]])))        # pred == truth: the diagonal equals the voxels
    assert not match.match_volumes(*(dev(v) for v in R.case('disjoint'))).overlap.any()
    assert not match.match_volumes(*(dev(v) for v in R.case('empty'))).overlap.any()
    inner = host(match.match_volumes(*(dev(v) for v in R.case('inner_runs'))).overlap)
    assert inner[0, :2, :2].tolist() == [[18, 0], [0, 18]] and inner[1, :2, :2].tolist() == [[18, 0], [0, 18]] and inner.sum() == 72
    rest = host(match.match_volumes(*(dev(v) for v in R.case('thirty_four'))).overlap)[0]
    assert rest[32, 32] == 8 and rest[:32, :32].sum() == 32 * 4 and rest.sum() == 34 * 4           # ranking ties by first voxel fill the rest cell


def test_the_same_tensor_on_both_sides():
    pred, _ = R.case('seeded_5x37x63')
    d = dev(pred)
    m = match.match_volumes(d, d, across='full')
    assert_equal_tables(m, R.tables(pred, pred, 'full'), 'pred is truth')
    assert torch.equal(m.nles[:, 0], m.nles[:, 1]) and torch.equal(m.top[:, 0], m.top[:, 1])
    assert torch.equal(m.frames[:, :, 0], m.frames[:, :, 1]) and torch.equal(m.frames[:, :, 0], m.frames[:, :, 2])


def test_non_contiguous_and_transposed_inputs():
    pred, truth = R.case('seeded_5x37x63')
    wide_p, wide_t = torch.zeros((5, 37, 63, 9), device='cuda'), torch.zeros((5, 37, 63, 9), device='cuda')
    wide_p[..., 1::2], wide_t[..., 1::2] = dev(pred), dev(truth)
    m = match.match_volumes(wide_p[..., 1::2], wide_t[..., 1::2])                                 # a strided view of the channels
    assert_equal_tables(m, R.case_tables('seeded_5x37x63', 'overlap'), 'strided')
    tp, tt = np.ascontiguousarray(pred.transpose(0, 2, 1, 3)), np.ascontiguousarray(truth.transpose(0, 2, 1, 3))
    m = match.match_volumes(dev(pred).permute(0, 2, 1, 3), dev(truth).permute(0, 2, 1, 3), across='full')      # [N, W, H, C] views
    assert_equal_tables(m, R.tables(tp, tt, 'full'), 'transposed')


# ---- 2. chunking
def test_channel_by_channel_equals_all_channels():
    name = 'seeded_5x37x63'
    pred, truth = R.case(name)
    n, h, w, c = pred.shape
    dp, dt = dev(pred), dev(truth)
    lib = L.lib()
    one, every = int(lib.octseg_match_scratch_bytes(1, n, h, w)), int(lib.octseg_match_scratch_bytes(c, n, h, w))
    assert one < every
    for across in ACROSS:
        whole = match.match_volumes(dp, dt, across=across)
        for budget in (one, every - 1):
            part = match.match_volumes(dp, dt, across=across, scratch_bytes=budget)
            assert all(torch.equal(a, b) for a, b in zip(whole, part))
            assert_equal_tables(part, R.case_tables(name, across), f'budget {budget}')
    with pytest.raises(ValueError, match=str(one)):                      # not even one channel fits: the need is named
        match.match_volumes(dp, dt, scratch_bytes=one - 1)


# ---- 3. the scratch is work space only, outputs stay inside their extents, refused calls write nothing
def test_scratch_fills_guard_bands_and_refusals():
    name = 'straddle'
    pred, truth = R.case(name)
    n, h, w, c = pred.shape
    dp, dt = dev(pred), dev(truth)
    lib = L.lib()
    need = int(lib.octseg_match_scratch_bytes(c, n, h, w))
    s = L.stream_ptr()
    nles = torch.full((c + 1, 2), 7, dtype=torch.int32, device='cuda')
    top = torch.full((c + 1, 2, 32, 8), 7, dtype=torch.int32, device='cuda')
    overlap = torch.full((c + 1, 33, 33), 7, dtype=torch.int32, device='cuda')
    frames = torch.full((c + 1, n, 3), 7, dtype=torch.int32, device='cuda')
    scratch = torch.empty((need + 8,), dtype=torch.uint8, device='cuda')

    def call(p=L.ptr(dp), t=L.ptr(dt), nn=n, hh=h, ch=c, across=0, scr=L.ptr(scratch), nbytes=need, nl=L.ptr(nles), ov=L.ptr(overlap)):
        return lib.octseg_volume_match(p, t, nn, hh, w, ch, across, scr, nbytes, nl, L.ptr(top), ov, L.ptr(frames), s)

    # refused calls first: nothing may be written
    assert call(p=None) == -5 and call(t=None) == -5 and call(scr=None) == -5 and call(nl=None) == -5 and call(ov=None) == -5
    assert call(nbytes=need - 1) == -5 and call(across=2) == -5 and call(scr=L.ptr(scratch[4:])) == -5
    assert call(hh=0) == -1 and call(ch=17) == -1 and call(nn=0) == -1 and call(ch=0) == -1
    torch.cuda.synchronize()
    assert (nles == 7).all() and (top == 7).all() and (overlap == 7).all() and (frames == 7).all()
    gen = torch.Generator(device='cuda').manual_seed(3)
    for across in (0, 1):
        want = R.case_tables(name, ACROSS[across])
        got = []
        for fill in (0x00, 0xFF, 'random'):
            if fill == 'random':
                scratch.copy_(torch.randint(0, 256, (need + 8,), dtype=torch.uint8, device='cuda', generator=gen))
            else:
                scratch.fill_(fill)
            for t in (nles, top, overlap, frames):
                t.fill_(7)
            L.check(call(across=across))
            got.append([host(nles[:c]), host(top[:c]), host(overlap[:c]), host(frames[:c])])
            assert_equal_tables(got[-1], want, f'fill {fill}')
            assert (nles[c] == 7).all() and (top[c] == 7).all() and (overlap[c] == 7).all() and (frames[c] == 7).all()      # the guard rows
        for g in got[1:]:
            assert all(np.array_equal(a, b) for a, b in zip(g, got[0]))
    assert np.array_equal(host(dp), pred) and np.array_equal(host(dt), truth)


def test_wrappers_refuse_mismatched_stacks():
    a, b = torch.zeros((2, 4, 4, 4), device='cuda'), torch.zeros((2, 4, 5, 4), device='cuda')
    with pytest.raises(ValueError, match='agree in shape'):
        match.match_volumes(a, b)
    with pytest.raises(ValueError, match='agree in shape'):
        match.match_volumes(a, a[..., :3])
    for bad in (torch.zeros((2, 4, 4, 17), device='cuda'), torch.zeros((2, 0, 4, 4), device='cuda'), a.double(), a[0]):
        with pytest.raises(ValueError):
            match.match_volumes(bad, bad)
    with pytest.raises(ValueError, match='across'):
        match.match_volumes(a, a, across='6')


# ---- 4. the report and the command line
def test_match_report_equals_build_match_of_the_reference_tables():
    for name, across, kw in (('seeded_5x70x129', 'overlap', {}), ('thirty_four', 'full', {'iou': 0.6}),
                             ('cover_two', 'overlap', {'criterion': 'overlap', 'min_overlap': 3, 'min_pixels': 2})):
        pred, truth = R.case(name)
        n, h, w, c = pred.shape
        names = [f'f{i}' for i in range(n)]
        classes = [f'k{i}' for i in range(c)]
        rep = match.match_report(dev(pred), dev(truth), image_names=names, classes=classes, across=across, **kw)
        want = R.case_tables(name, across)
        assert rep == match.build_match(*want, h, w, image_names=names, classes=classes, **kw)
        assert json.loads(json.dumps(rep)) == rep
        R.assert_report_equals_scores(rep, R.scores(*want, **kw), classes)
    rep = match.match_report(*(dev(v) for v in R.case('thirty_four')), classes=['c'])
    assert rep['c']['truncated'] is True and rep['c']['n_pred'] == 34 and rep['c']['unranked_overlap'] == {'pred_rest': 8, 'truth_rest': 8}
    rep = match.match_report(*(dev(v) for v in R.case('cover_two')), classes=['m', 's'])
    assert rep['m']['merged'] == 1 and rep['m']['split'] == 0 and rep['s']['split'] == 1 and rep['s']['merged'] == 0


def test_main_writes_lesion_match_json(tmp_path, capsys):
    pred_dir, truth_dir, save_dir = tmp_path / 'pred', tmp_path / 'truth', tmp_path / 'out'
    pred_dir.mkdir()
    truth_dir.mkdir()
    pred, truth = R.case('seeded_2x9x64')
    for folder, st in ((pred_dir, pred), (truth_dir, truth)):
        for i in range(2):
            Image.fromarray((st[i] * 255).astype(np.uint8)).save(str(folder / f's{i}.tiff'))
    report = match.main([str(pred_dir), str(truth_dir), str(save_dir), 'across=full'])
    path = save_dir / 'lesion_match.json'
    assert capsys.readouterr().out.strip() == str(path)
    saved = json.load(open(path))
    classes = ['Lumen', 'Fibrous cap', 'Lipid core', 'Vasa vasorum']
    want = {'images': ['s0.tiff', 's1.tiff'], 'classes': classes, 'across': 'full', 'unit': 'voxel',
            'match': match.build_match(*R.case_tables('seeded_2x9x64', 'full'), 9, 64, image_names=['s0.tiff', 's1.tiff'], classes=classes)}
    assert saved == json.loads(json.dumps(want)) == json.loads(json.dumps(report))
